/*
 * uavqp.h -- C ABI of the MI355X-native batched minimum-jerk / minimum-snap trajectory QP back-end.
 *
 * Drop-in boundary for ONE hot path of peiyu-cui/uav_motion_planning: the polynomial-trajectory QP
 * of traj_optimization::MinimumControl (reference: src/planner/traj_optimization/include/
 * traj_optimization/minimum_control.h:10-48, src/minimum_control.cpp:5-202).  The reference has no
 * FFI; its interface for this path is the C++ class, so the bindings a maintainer adds are the two
 * C++ facades in uav_motion_planning_amd/cpp/ (MinimumControl, TrajOptimizer) -- see INTEGRATION.md.
 *
 * Plain pointers and sizes only: no Eigen, STL, torch or HIP types cross this boundary.
 * All floating-point data is IEEE float64 (the reference's c_float/VectorXd type); indices int32.
 *
 * -------------------------------------------------------------------------------------------------
 * Problem solved per trajectory and per axis (r = 3 min-jerk: the reference; r = 4 min-snap):
 *   minimise   sum_i  integral_0^{T_i} (d^r p_i/dt^r)^2 dt          [getHessian,  minimum_control.cpp:5-19]
 *   subject to p_0^(d)(0)   = start derivative d, d = 0..r-1        [rows 0..r-1,          :29-31, :101-107]
 *              p_i(T_i)     = waypoint i+1                          [waypoint rows,        :34-42, :118-124]
 *              p_i^(d)(T_i) = p_{i+1}^(d)(0), d = 0..r-1            [continuity rows,      :45-74]
 *              p_{M-1}^(d)(T) = end derivative d                    [end rows,             :77-95, :109-115]
 * Every row is an equality (lb == ub in the reference), so the QP has a unique minimiser; the device
 * path computes that minimiser directly (reduced SPD block-tridiagonal system)
 * instead of iterating ADMM to OSQP's eps = 1e-3.
 *
 * Data layout (one batch = n_traj independent trajectories, 3 axes each):
 *   seg_offsets [n_traj+1] int32   CSR offsets into the segment arrays; trajectory b has
 *                                  M_b = seg_offsets[b+1]-seg_offsets[b] segments and M_b+1 waypoints.
 *                                  May be NULL when uniform_segments > 0 (then M_b = uniform_segments).
 *   waypoints   [sum_b (M_b+1)][3] xyz interleaved, trajectory b starts at row seg_offsets[b] + b
 *                                  (= what A* / RRT* hand over: std::vector<Eigen::Vector3d>,
 *                                  test_minimum_jerk.cpp:41-57).
 *   times       [sum_b M_b]        segment durations (time_vec, test_minimum_jerk.cpp:65-71), > 0.
 *   bc          [n_traj][2][r-1][3] boundary derivatives: [start|end][vel,acc(,jerk)][xyz]
 *                                  (bound_vel / bound_acc of MinimumControl::solve, minimum_control.h:32-35).
 *   coeff_out   [sum_b 3*M_b*2r]   trajectory b at 3*2r*seg_offsets[b], layout [axis][segment][2r]:
 *                                  each [axis] slice IS the reference's coef_1d_ vector for that axis --
 *                                  coef[2r*i + k] multiplies t^k (ascending powers) in segment-local time
 *                                  (minimum_control.cpp:186, consumer poly_traj_server.cpp:68-78).
 *   status_out  [n_traj] int32     UAVQP_SOLVED or a negative per-trajectory code (may be NULL).
 */
#ifndef UAVQP_H_
#define UAVQP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uavqp_ctx uavqp_ctx;

/* return codes of every entry point (never throws) */
enum {
    UAVQP_OK = 0,
    UAVQP_ERR_INVALID_ARG = -1,
    UAVQP_ERR_HIP = -2,       /* HIP runtime error; uavqp_last_error() has the text */
    UAVQP_ERR_NO_DEVICE = -3, /* no usable gfx950 device: the product path never falls back to CPU */
    UAVQP_ERR_ALLOC = -4,
    UAVQP_ERR_RCCL = -5       /* RCCL missing or a collective failed; uavqp_last_error() has the text */
};

/* per-trajectory status (positive = OSQP's OSQP_SOLVED value, which the reference's solve() maps to true) */
enum {
    UAVQP_SOLVED = 1,
    UAVQP_MAX_ITER_REACHED = -2, /* inequality-constrained solves only (OSQP's OSQP_MAX_ITER_REACHED value): iteration cap reached, or a
                                  * working set went singular and could neither be repaired nor certified infeasible (undecided) */
    UAVQP_PRIMAL_INFEASIBLE = -3, /* general-rows solve only (OSQP's OSQP_PRIMAL_INFEASIBLE value): the rows have no common point, proven
                                   * by a Farkas certificate that passes OSQP's test at uavqp_settings.eps_prim_inf */
    UAVQP_INVALID_INPUT = -10, /* M < 1, M > max_segments, T <= 0 or non-finite input */
    UAVQP_NON_FINITE = -11     /* solution overflowed / NaN (pathological time allocation) */
};

const char* uavqp_version(void);
const char* uavqp_last_error(void);

/* Replaces construction of traj_optimization::MinimumControl + OsqpEigen::Solver
 * (minimum_control.h:14,44).  One ctx per host thread / device; owns a HIP stream and workspaces.  The owned stream is
 * a blocking stream, i.e. ordered with the legacy default (NULL) stream: buffers filled or read there need no extra
 * synchronisation.  A stream passed through uavqp_set_stream is used as it is. */
int uavqp_create(uavqp_ctx** out_ctx, int device);
int uavqp_destroy(uavqp_ctx* ctx);

/* Run all subsequent device work of this ctx on an existing hipStream_t (e.g. the caller's compute
 * stream).  NULL restores the ctx-owned stream.  The ctx's sweep workspaces are shared by its calls and
 * ordered by the stream: work still in flight on the previous stream must be complete before switching
 * (uavqp_synchronize), and concurrent streams need one ctx each. */
int uavqp_set_stream(uavqp_ctx* ctx, void* hip_stream);
int uavqp_synchronize(uavqp_ctx* ctx);

/* Kernel variant selection: 0 = auto, 1 = generic lane-per-trajectory kernel, 2 = register-resident
 * specialised kernel (uniform batches only, tile shape chosen by batch size); 4 / 8 / 16 / 32 = specialised
 * kernel with that many trajectories per wave (4: two lane pairs per axis, the smallest batches; 8: one lane
 * pair per axis, latency shape; 16 / 32: one lane pair per trajectory).
 * For benchmarking/tests; results agree to rounding. */
int uavqp_set_variant(uavqp_ctx* ctx, int variant);

/* Solver settings: plain C struct, replaces the OsqpEigen settings calls of the reference
 * (minimum_control.cpp:160-162: setWarmStart(true), setPrimalInfeasibilityTollerance(1e-3), setMaxIteration(1000))
 * and every tuning knob of this back-end.  uavqp_default_settings fills the defaults (= the reference's three values
 * plus this back-end's measured choices); uavqp_set_settings validates and stores a copy in the ctx, uavqp_get_settings
 * reads it back.  Nothing on the launch path reads the environment: the UAVQP_* variables listed in INTEGRATION.md are
 * read ONCE, by uavqp_create, as overrides of the defaults.
 *   struct_size            sizeof(uavqp_settings) of the caller's build (versioning; must be set)
 *   warm_start             reference: true.  The equality-constrained solve is direct (nothing to warm-start); for the
 *                          inequality-constrained entry points it is the default of their warm_start argument semantics:
 *                          uavqp_solve_corridor_warm_device's explicit argument wins.  Kept for API parity.
 *   eps_prim_inf           reference: 1e-3 (OSQP's primal-infeasibility tolerance, the one tolerance the reference sets).  OSQP calls a problem
 *                          primal infeasible when its dual increment dy satisfies |A' dy|_inf <= eps |dy|_inf and
 *                          u' max(dy, 0) + l' min(dy, 0) <= -eps |dy|_inf.  The general-rows solve applies exactly that test to the Farkas
 *                          certificate its dual active-set method ends with when a violated row depends on the working set and no
 *                          multiplier blocks (dy = the dependency's coefficients, value = minus the row's violation): accepted ->
 *                          UAVQP_PRIMAL_INFEASIBLE; a certificate below the margin -> UAVQP_MAX_ITER_REACHED (undecided, as OSQP would run
 *                          into its iteration cap).  Smaller eps: every provable infeasibility is reported.  (lo > hi on one row or box is
 *                          rejected up front, UAVQP_INVALID_INPUT, as OSQP's data validation does.)  Knot boxes alone are always feasible.
 *   max_iter               reference: 1000 (ADMM iterations).  Here: cap on active-set iterations of the
 *                          inequality-constrained solves; <= 0 = automatic (8 * max_segments + 20).  Hitting it yields
 *                          UAVQP_MAX_ITER_REACHED with a feasible, smooth trajectory (as OSQP's status of the same name).
 *   kernel_variant         as uavqp_set_variant (0 auto)
 *   ragged_window_sort     1: ragged batches >= 2048 are dealt to lanes by segment count inside windows (default; since round 6 the waves of the
 *                          lane-pair kernel rank their window themselves, up to 63 segments), 2: the same dealing from its own launch in front of
 *                          the solve (rounds 2-5; results identical), 0: lane order
 *   generic_lanes_per_traj 0 auto, 1 = one lane per trajectory, 2 = a lane pair per trajectory (two-sided elimination),
 *                          3 = one lane per (trajectory, axis)
 *   generic_waves_per_cu   0 auto, > 0: resident waves per CU of the generic kernel
 *   corridor_pdas_rounds   block-pivoting rounds before the single-pivot active-set phase of a COLD corridor solve (default 3; not
 *                          used with corridor_initial_guess = 2, whose starting set only has to be verified)
 *   corridor_pdas_rounds_warm  the same for a warm-started one (default 0: measured on config 5's outer loop, block rounds from
 *                          the carried working set only disturb it -- largest iteration counts 57 / 54 / 37 / 27 with 3 rounds, 41 / 43 /
 *                          22 / 12 with none and the previous positions as the starting point)
 *   corridor_initial_guess working set a COLD corridor solve starts from.  2 (default): the set a dual active-set method in position space ends
 *                          with (qp_corridor_dual.h, DESIGN.md section 5.13: inverse Hessian of the knot positions once per trajectory,
 *                          Goldfarb-Idnani on a swept tableau) -- the exact block solve then verifies it, one solve per problem instead of
 *                          ~12; trajectories of up to 33 segments, longer batches fall back to 1.  1: the knots whose boxes the end-state
 *                          polynomial misses (closed form, section 5.4).  0: the empty set.  Same result to the last bit whichever is used, for every
 *                          problem that ends UAVQP_SOLVED (one that runs into max_iter hands back the iterate it stopped at, which depends on the start).
 *   rows_lanes_per_problem uavqp_solve_rows_batch_*: 0 auto / 2 = a lane pair per (trajectory, axis) problem with the sweep state in LDS
 *                          (default), 1 = one lane per problem, state in an HBM workspace (the round-2 kernel, kept for A/B).  Same result.
 *   corridor_tail_shape    1 (default): small batches of long r = 4 corridor problems run two waves per CU with twice the sweep state on
 *                          chip (shorter iterations: such a solve is as slow as its slowest problem); 0: always four waves per CU.  Same result.
 *   corridor_prelude_lanes lanes per trajectory of the dual prelude of a cold corridor solve (corridor_initial_guess = 2): 0 (default) / 8 = groups of
 *                          8 or 16 lanes (qp_corridor_dual.h); 1 = ONE lane per trajectory with its tableau in lane-private LDS, single precision
 *                          (qp_corridor_lane.h; batches of at most 16 segments per trajectory, else the groups) -- built in round 5 to get rid of
 *                          the replicated chain and the lockstep of eight, measured at parity on config 3 (330 vs 338 us: a per-lane pivot costs
 *                          ~2.5 k instructions of selects per trip), kept as the independent cross-check of the prelude.  Same result.
 *   cloud_window           1 (default): uavqp_corridor_from_cloud_device sorts rows and points along the cloud's longest axis and scans,
 *                          per block of neighbouring rows, only the points that can still change a box (large clouds, no clearance
 *                          output); rows whose distance to the cloud's bounding box already exceeds the cap of the clearance are
 *                          not scanned at all (an exact bound: Cauchy-Schwarz on the robot ellipsoid's metric); 0: always the
 *                          exhaustive scan.  2 / 3: the two experiments of round 5 on a 2-D grid over the cloud (rings of cells
 *                          around a row; a near pass + a far pass over rows bucketed by the radius they still need) -- both measured
 *                          slower than 1 on BASELINE config 5 (1.23 / 1.25 ms against 0.61 ms per call), kept as cross-checks.
 *                          Identical boxes with every value.
 *   realloc_dead_band      uavqp_time_reallocate_device stretches only when the limit ratio exceeds this (default 1.01)
 *   realloc_overshoot      ... and then by overshoot * ratio (default 1.02) */
typedef struct uavqp_settings {
    int32_t struct_size;
    int32_t warm_start;
    double eps_prim_inf;
    int32_t max_iter;
    int32_t kernel_variant;
    int32_t ragged_window_sort;
    int32_t generic_lanes_per_traj;
    int32_t generic_waves_per_cu;
    int32_t corridor_pdas_rounds;
    int32_t corridor_initial_guess;
    int32_t rows_lanes_per_problem;
    int32_t corridor_pdas_rounds_warm;
    int32_t cloud_window;
    int32_t corridor_tail_shape;
    int32_t corridor_prelude_lanes;   /* (sits in what was padding: sizeof(uavqp_settings) is unchanged) */
    double realloc_dead_band;
    double realloc_overshoot;
} uavqp_settings;
void uavqp_default_settings(uavqp_settings* out);
int uavqp_set_settings(uavqp_ctx* ctx, const uavqp_settings* settings);
int uavqp_get_settings(const uavqp_ctx* ctx, uavqp_settings* out);

/* Batched solve, DEVICE pointers, asynchronous on the ctx stream.
 * Replaces, for a whole batch and 3 axes at once, MinimumControl::solve + getCoef1d
 * (minimum_control.cpp:127-192, :199-202).
 *   r                 3 (min-jerk, reference) or 4 (min-snap)
 *   uniform_segments  > 0: every trajectory has that many segments (seg_offsets may be NULL)
 *                     0  : ragged batch, seg_offsets required
 *   max_segments      upper bound on M_b (ragged); ignored for uniform batches                    */
int uavqp_solve_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                             const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                             const double* d_bc, double* d_coeff_out, int32_t* d_status_out);

/* Same with HOST pointers: H2D copy, solve, D2H copy, synchronous.  total_segments = sum_b M_b.
 * The coefficients of a trajectory flagged UAVQP_INVALID_INPUT come back as zeros (the device entry leaves them
 * untouched; the host entries clear their staging buffer first -- both host entries behave the same); a
 * UAVQP_NON_FINITE trajectory carries the non-finite values it overflowed to.
 * Argument checks shared by every *_host entry (one staging routine, csrc/uavqp_stage.h): ragged offsets start at 0 and never decrease;
 * a trajectory longer than a positive max_segments is flagged UAVQP_INVALID_INPUT, not refused; a batch whose waypoint rows
 * (total_segments + n_traj) do not fit an int is UAVQP_ERR_INVALID_ARG; optional outputs may be NULL; n_traj == 0 is a no-op. */
int uavqp_solve_batch_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                           const int32_t* seg_offsets, const double* waypoints, const double* times,
                           const double* bc, double* coeff_out, int32_t* status_out);

/* Single-axis entry with the exact argument meaning of
 *   bool MinimumControl::solve(VectorXd& pos_1d, Vector2d& bound_vel, Vector2d& bound_acc, VectorXd& time_vec)
 * (minimum_control.h:32-35): pos_1d[n_seg+1], bound_*[2] = (start, end), time_vec[n_seg]; writes
 * coef_1d[2r*n_seg].  bound_jerk is read only when r == 4 (NULL = zeros).  Host pointers, synchronous.
 * Returns UAVQP_OK and *status_out = UAVQP_SOLVED on success. */
int uavqp_solve_axis_host(uavqp_ctx* ctx, int r, int n_seg, const double* pos_1d, const double* bound_vel,
                          const double* bound_acc, const double* bound_jerk, const double* time_vec,
                          double* coef_1d, int32_t* status_out);

/* Corridor-constrained batched solve (north-star extension, BASELINE configs 3 and 5; no reference
 * counterpart: every row of the reference QP is an equality, minimum_control.cpp:98-125,146-147).
 * The interior-waypoint rows p_i(T_i) = w_{i+1} (minimum_control.cpp:34-42,118-124) become
 * corr_lo <= p_i(T_i) <= corr_hi per axis; everything else is unchanged.
 *   d_corr_lo / d_corr_hi  [sum_b (M_b+1)][3], same indexing as waypoints; the entries of the first and last
 *                          waypoint of a trajectory are ignored (start/end positions stay equalities);
 *                          lo == hi pins that waypoint (so lo = hi = waypoints reproduces uavqp_solve_batch_device).
 *   d_waypoints            start/end positions, and the initial guess (clipped into the box) elsewhere.
 *   d_iters_out            [n_traj] active-set iterations (max over axes), may be NULL.
 * Asynchronous for uniform batches; for a RAGGED batch the device entry points read the last CSR offset back first (4 bytes, one
 * stream synchronisation: workspaces are sized by the batch's total segment count) -- the host entries and the pipeline, which know
 * the total, do not.
 * Exact primal active-set solve in the Hermite variables; status UAVQP_MAX_ITER_REACHED
 * (uavqp_settings.max_iter, default 8 M + 20 iterations) leaves a feasible, smooth, possibly sub-optimal trajectory.
 * M <= 63; a longer trajectory is flagged UAVQP_INVALID_INPUT (the working set is one 64-bit word per axis). */
int uavqp_solve_corridor_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                      const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                                      const double* d_bc, const double* d_corr_lo, const double* d_corr_hi,
                                      double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out);
int uavqp_solve_corridor_batch_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                    const int32_t* seg_offsets, const double* waypoints, const double* times,
                                    const double* bc, const double* corr_lo, const double* corr_hi,
                                    double* coeff_out, int32_t* status_out, int32_t* iters_out);

/* Warm-started corridor solve for outer loops (BASELINE config 5: the corridor QP is re-solved after every time
 * re-allocation, and its working set barely moves).  Same problem, same result as uavqp_solve_corridor_batch_device;
 * d_active_set [n_traj][3][2] uint64 holds per (trajectory, axis) the working set of the active-set method: word 0
 * bit k = the box of interior waypoint k (1 <= k <= M-1 <= 62) is active, word 1 bit k = at its upper bound.
 * M <= 63; a longer trajectory is flagged UAVQP_INVALID_INPUT.
 *   warm_start == 0: the buffer is only written (working set at the solution);
 *   warm_start != 0: it is read as the initial working set (any bit pattern is a valid guess: wrong guesses cost
 *                    iterations, never correctness) and overwritten with the final one.
 *   warm_start == 2: in addition d_coeff_out is READ first: it holds the polynomials of the previous solve of the same batch
 *                    (same boxes, e.g. other durations), and the feasible starting point of the active-set method takes its free
 *                    positions from their knot positions (clipped into the boxes -- any content is admissible) instead of the
 *                    waypoints: a start close to the new minimiser is blocked by few bounds on its way there.
 * A trajectory that ends UAVQP_MAX_ITER_REACHED writes an empty set.  No reference counterpart. */
int uavqp_solve_corridor_warm_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                     const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                                     const double* d_bc, const double* d_corr_lo, const double* d_corr_hi,
                                     double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out,
                                     uint64_t* d_active_set, int warm_start);

/* GENERAL inequality rows (north-star extension: the reference hands any l <= A x <= u to OSQP, minimum_control.cpp:146-147,
 * 164-180, but only ever builds equality rows, :98-125).  On top of the knot boxes of uavqp_solve_corridor_batch_device every
 * segment carries up to rows_per_segment (1 or 2) rows
 *       row_lo <= p_i^(d)(tau T_i) <= row_hi      per axis,   d = 0 position, 1 velocity, 2 acceleration (, 3 jerk for r = 4)
 * i.e. position samples at in-segment times (BASELINE config 3's "K = 2 mid-segment samples"), per-axis velocity / acceleration
 * limits, or -- through the monomial basis -- any row a' c_i on the coefficients of one segment.  This is the ORIGINAL spline
 * space (adapters.refine_with_mid_knots inserts knots instead: cheaper -- it runs on the corridor solver -- but a larger space).
 *   d_corr_lo / d_corr_hi  knot boxes as in uavqp_solve_corridor_batch_device, or both NULL: the reference's waypoint equalities
 *   d_row_tau    [sum_b M_b][rows_per_segment]     position of the row in its segment as a fraction of T_i, 0 <= tau < 1
 *                                                  (tau = 0 with d >= 1 is a limit on a knot derivative; tau = 0, d = 0 is the knot box: rejected)
 *   d_row_deriv  [sum_b M_b][rows_per_segment]     int32 derivative order d, < 0: slot unused
 *   d_row_lo / d_row_hi [sum_b M_b][rows_per_segment][3]   bounds per axis (lo == hi: an equality row; +-1e300 for a one-sided row)
 *   d_active_out [n_traj][3][2 + 2 rows_per_segment] uint64 (may be NULL): working set at the solution -- word 0 / 1: knot boxes
 *                active / at the upper bound (bit k = interior waypoint k), then per row slot j words 2+2j / 3+2j (bit i = segment i)
 * Exact dual active-set solve (Goldfarb-Idnani on the block-tridiagonal KKT system with the rows' multipliers riding in the knot
 * blocks): no feasible starting point is needed, the result is the QP's minimiser to rounding.  A row that enters and turns
 * out to depend on the working set (the KKT system goes singular: rows that no free unknown can move, duplicated or contradictory
 * rows, a degenerate vertex) takes the method's zero-primal-step route: the multipliers move along the dependency until one of the
 * working set reaches zero -- that constraint leaves, the solve goes on (degenerate but feasible problems are SOLVED) -- or none does:
 * a Farkas certificate, status UAVQP_PRIMAL_INFEASIBLE if it passes OSQP's test at uavqp_settings.eps_prim_inf (the reference's 1e-3,
 * minimum_control.cpp:161), else UAVQP_MAX_ITER_REACHED.  UAVQP_MAX_ITER_REACHED also ends a problem at uavqp_settings.max_iter (default
 * 12 M (1 + rows_per_segment) + 30) and one whose working set is regular but too ill-conditioned for the block solve (undecided: the direction
 * solve that would yield the certificate does not vanish, |diag(H) z| > max(eps_prim_inf, 1e-6) |dy| -- the one class of problems the OSQP port proves
 * infeasible and this back-end leaves undecided: 2 of 1246 infeasible soak draws at the reference's eps_prim_inf = 1e-3, 14 at 1e-9, profiles/r06_soak.txt;
 * a feasible problem is never called infeasible).  Both
 * statuses hand back the minimiser of the last regular working set, which need NOT satisfy the remaining rows.  A single-segment
 * trajectory has no free unknown at all: its rows are only checked (violated -> UAVQP_PRIMAL_INFEASIBLE).  M <= 63.
 * Asynchronous for uniform batches; a ragged batch costs one 4-byte read-back + stream synchronisation (see uavqp_solve_corridor_batch_device). */
int uavqp_solve_rows_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                  const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                                  const double* d_bc, const double* d_corr_lo, const double* d_corr_hi, int rows_per_segment,
                                  const double* d_row_tau, const int32_t* d_row_deriv, const double* d_row_lo,
                                  const double* d_row_hi, double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out,
                                  uint64_t* d_active_out);
/* The same solve from HOST pointers (staged through device memory, synchronous; a trajectory flagged UAVQP_INVALID_INPUT comes back
 * as zeros, a UAVQP_MAX_ITER_REACHED / UAVQP_PRIMAL_INFEASIBLE one carries the minimiser of its last regular working set -- which need NOT
 * satisfy the remaining rows: check the status, not the coefficients): what a caller of the reference's solver interface has -- it hands its rows to OSQP from host memory,
 * minimum_control.cpp:164-170. */
int uavqp_solve_rows_batch_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                const int32_t* seg_offsets, const double* waypoints, const double* times, const double* bc,
                                const double* corr_lo, const double* corr_hi, int rows_per_segment, const double* row_tau,
                                const int32_t* row_deriv, const double* row_lo, const double* row_hi, double* coeff_out,
                                int32_t* status_out, int32_t* iters_out);

/* Time re-allocation step of the outer loop of BASELINE config 5 (north-star extension; the reference uses a
 * constant 1.0 s per segment, test_minimum_jerk.cpp:65-71, and has no such loop -- nothing to mirror, parity is
 * per inner solve).  The 3-axis speed |v| and acceleration |a| of the solved polynomials are sampled at
 * samples_per_seg + 1 uniform points per segment; with rho = max(|v|_peak / v_max, sqrt(|a|_peak / a_max)) over the
 * whole trajectory, if rho > 1.01 EVERY duration of that trajectory is scaled by min(max_stretch, 1.02 rho)
 * (dead band 1.01 and overshoot 1.02 are uavqp_settings.realloc_dead_band / realloc_overshoot)
 * (never shrunk).  Scaling is per trajectory, not per segment: stretching one segment next to short ones makes
 * it overshoot more (it inherits their knot acceleration) and diverges; uniform scaling T -> sT lowers speeds
 * ~1/s and accelerations ~1/s^2.
 * Non-finite input: if ANY sample of a trajectory is NaN or infinite (coefficients or durations that a UAVQP_NON_FINITE solve
 * hands over), the whole trajectory is left unchanged and d_changed_out[b] = 0, whatever its other segments say.
 * d_times is updated in place; d_changed_out[b] (may be NULL) receives the number of stretched segments of
 * trajectory b, so the caller can stop when it is all zero.  Typical loop: solve, reallocate, solve, ... (<= 5x). */
int uavqp_time_reallocate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                 double* d_times, const double* d_coeff, double v_max, double a_max,
                                 int samples_per_seg, double max_stretch, int32_t* d_changed_out);

/* Control cost of solved trajectories and its EXACT gradient with respect to the segment durations (no reference counterpart as a
 * function: OSQP reports obj_val = 1/2 x' P x per axis, the reference never reads it).  Per trajectory, from the coefficients a solve wrote:
 *   cost[b] = J_b = sum over axes and segments of integral_0^{T_i} (p_i^(r)(t))^2 dt = c' P c with the reference's P (getHessian,
 *             minimum_control.cpp:5-19; TWICE OSQP's objective value), by the closed-form blocks of P, not by quadrature;
 *   grad[seg_offsets[b] + i] = dJ_b / dT_i at the minimiser of the EQUALITY-constrained QP (uavqp_solve_batch_*):  dJ/dT_i = -H_i,
 *             H_i = (p^(r))^2 + 2 sum_{m=1}^{r-1} (-1)^m p^(r+m) p^(r-m), summed over the three axes, evaluated at the segment's local
 *             time 0 where p^(k)(0) = k! c_k (H is constant along a segment).  r = 3: H = j^2 - 2 s a + 2 c v with v, a, j, s, c =
 *             c1, 2 c2, 6 c3, 24 c4, 120 c5.  (Envelope theorem in the knot-derivative variables: the constraints do not depend on T there
 *             and each segment is the unique degree-(2r-1) interpolant of its two knot states.)
 * The gradient is that of the OPTIMAL cost: meaningful for coefficients of uavqp_solve_batch_* at d_times (it also holds for knot boxes;
 * it does NOT hold for rows at a fraction of T_i -- corridor and general-rows solves are out of scope here).  d_cost [n_traj] / d_grad
 * [sum_b M_b]: either may be NULL.  The order of the additions is fixed: the same bits run to run.  Asynchronous on the ctx stream, no
 * allocation. */
int uavqp_cost_time_gradient_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                    const double* d_times, const double* d_coeff, double* d_cost, double* d_grad);

/* Optimisation of the DISTRIBUTION of time over the segments (north-star extension; the reference uses a constant 1.0 s per segment,
 * test_minimum_jerk.cpp:65-71, and has no such loop -- nothing to mirror, parity is per inner solve).  Per trajectory
 *       minimise  f(T) = J(T) + time_weight * sum_i T_i     subject to  t_min <= T_i <= t_max,
 * J(T) the cost above at the minimiser of the equality-constrained QP for durations T.  Method: projected gradient descent in
 * u_i = log T_i (direction d_i = T_i (dJ/dT_i + time_weight), zero where a bound blocks it; T stays positive and the problem is far better
 * conditioned than in T: J scales like T^-(2r-1)) with Armijo backtracking: a trial T_i exp(-alpha d_i), clamped into the bounds, is
 * accepted iff its solve ends UAVQP_SOLVED and f_trial <= f - armijo_c * sum_i d_i (u_i - u_trial_i); accepted: alpha *= grow, rejected:
 * alpha *= shrink.  The first alpha makes the largest |alpha d_i| equal to initial_step.  f never increases.
 * Host-side C++ sequencing of   clamp, solve, step, max_iters x { uavqp_solve_batch_device at the trial durations, step }, solve:
 * the accept / reject decision is taken per trajectory ON THE DEVICE, nothing is read back inside the loop, the number of launches depends
 * on max_iters alone.  Asynchronous on the ctx stream (a first call of a given size allocates the workspace).
 *   d_times          [total_segments] IN: the start, OUT: the accepted durations.  A trajectory whose durations are all positive and finite
 *                    has them projected into [t_min, t_max] first (that point is "the start"); a trajectory that is not UAVQP_SOLVED at the
 *                    start (e.g. a non-positive duration: UAVQP_INVALID_INPUT) keeps its status and its durations and takes no part.
 *   d_coeff_out      the solve AT the durations handed back: bit for bit what uavqp_solve_batch_device writes for them
 *   d_status_out     [n_traj] status of that solve (may be NULL)
 *   d_objective_out  [n_traj][2]: f at the start, f at the result (NaN, NaN for a trajectory that took no part)
 *   d_accepted_out   [n_traj] int32 accepted trials (may be NULL)
 *   params           uavqp_default_time_opt_params fills the defaults; UAVQP_ERR_INVALID_ARG for a wrong struct_size, max_iters < 0,
 *                    time_weight <= 0, t_min <= 0, t_min > t_max, initial_step <= 0, armijo_c outside (0, 1), shrink outside (0, 1), grow < 1
 *                    or a non-finite value.  max_iters = 0: the plain solve, both objective columns equal.
 * Velocity / acceleration limits: uavqp_time_optimize_limits_device below.
 * Out of scope: corridor and general-rows solves (see above), multi-GPU (shard the batch as for the solve: trajectories are independent). */
typedef struct uavqp_time_opt_params {
    int32_t struct_size;
    int32_t max_iters;      /* trials per trajectory (default 24) */
    double time_weight;     /* w > 0 (default 50) */
    double t_min;           /* bounds on every duration (default 0.01 ... 100 s) */
    double t_max;
    double initial_step;    /* largest change of log T_i in the first trial (default 0.1) */
    double armijo_c;        /* sufficient-decrease constant (default 1e-4) */
    double shrink;          /* step factor after a rejected trial (default 0.5) */
    double grow;            /* ... after an accepted one (default 2) */
} uavqp_time_opt_params;
void uavqp_default_time_opt_params(uavqp_time_opt_params* out);
int uavqp_time_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                               const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                               const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out,
                               double* d_objective_out, int32_t* d_accepted_out);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous; times is updated in place; the coefficients of a trajectory that is
 * not UAVQP_SOLVED come back as they do from uavqp_solve_batch_host). */
int uavqp_time_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                             const double* waypoints, double* times, const double* bc, const uavqp_time_opt_params* params,
                             double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out);

/* Backward pass of the equality-constrained solve (uavqp_solve_batch_*; no reference counterpart): the vector-Jacobian products of the
 * minimiser.  Per trajectory and axis c*(T, p, y0, yM) is the unique minimiser the forward solve returns (coeff_out layout
 * [axis][segment][2r]).  For a given g = dPhi/dc of an arbitrary Phi(c), in the same layout:
 *   grad_times[seg_offsets[b] + i] = sum over axes, j of g_j dc*_j/dT_i             [sum_b M_b]
 *   grad_waypoints[k][a]           = sum_j g_j dc*_j/dp_k (axis a)                  waypoint layout, all M_b + 1 knots incl. both ends
 *   grad_bc[b][s][d][a]            = sum_j g_j dc*_j/dbc                            bc layout [n_traj][2][r-1][3]
 * Equivalent KKT statement, per axis, with K = [[P, A'], [A, 0]], [c; nu] = K^-1 [0; b], [u; mu] = K^-1 [g; 0]:
 *   dPhi/dtheta = -u' (dP/dtheta c + dA'/dtheta nu) - mu' (dA/dtheta c) + mu' db/dtheta
 * (theta = T_i: b does not depend on it; theta = p_k or a boundary derivative: only b does).  This is ONLY the part through c*: the caller
 * adds the explicit T-dependence of its own loss (e.g. Phi = c' P(T) c has the explicit part c' dP/dT_i c = sum over axes of
 * (p^(r)(T_i))^2; with it the total is what uavqp_cost_time_gradient_device returns).
 * Computed in the knot-derivative variables of the forward solve: the adjoint system is the forward's SPD block-tridiagonal matrix
 * (DESIGN.md section 5.16), factorised once per trajectory with the three axes as right-hand sides; everything else is local to a segment.
 *   d_coeff        the coefficients uavqp_solve_batch_device wrote for these inputs
 *   d_status       [n_traj] its status, or NULL.  A trajectory whose status is not UAVQP_SOLVED, or that is invalid (M < 1, M > max_segments,
 *                  a duration that is not positive and finite) gets ZERO in all three outputs.
 *   d_grad_*       each may be NULL; all NULL: UAVQP_OK, nothing done.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a NULL input, ragged without offsets or with max_segments < 1, uniform with
 * total_segments != uniform_segments * n_traj.  One launch, asynchronous on the ctx stream, no read-back (a first call of a given size
 * grows the ctx workspace).  Every output element is written once, in a fixed order of additions: the same bytes run to run.
 * Out of scope: corridor and general-rows solves (active sets), multi-GPU (shard the batch as for the solve). */
int uavqp_solve_backward_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times, const double* d_bc,
                                const double* d_coeff, const int32_t* d_status, const double* d_grad_coeff, double* d_grad_times,
                                double* d_grad_waypoints, double* d_grad_bc);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_solve_backward_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                              const double* waypoints, const double* times, const double* bc, const double* coeff, const int32_t* status,
                              const double* grad_coeff, double* grad_times, double* grad_waypoints, double* grad_bc);

/* Velocity / acceleration limit penalty of solved trajectories with its gradients (no reference counterpart; a soft penalty on sampled
 * speed and acceleration in the style of GCOPTER / MINCO).  Per trajectory, K = samples_per_seg, tau_s = s / K, trapezoid weights
 * om_0 = om_K = 1/2, om_s = 1 otherwise, pos(x) = max(0, x):
 *   Phi = sum_i (T_i / K) sum_{s=0..K} om_s [ weight_v pos(|v_i(tau_s T_i)|^2 / v_max^2 - 1)^3 + weight_a pos(|a_i(tau_s T_i)|^2 / a_max^2 - 1)^3 ]
 * |.| the 3-axis norm of the segment's own polynomial at segment-local time.  The ratios are dimensionless: Phi has the unit of
 * time_weight * T, the two weights are comparable with uavqp_time_opt_params.time_weight; the cube makes Phi twice continuously differentiable.
 *   d_penalty     [n_traj] Phi
 *   d_grad_coeff  layout of coeff ([axis][segment][2r] per trajectory): dPhi/dc at FIXED durations
 *   d_grad_times  [sum_b M_b]: the EXPLICIT dPhi/dT_i at FIXED coefficients (the sampling times scale with T_i), with pv, pa the pos() terms:
 *                 Phi_i / T_i + (T_i / K) sum_s om_s tau_s [3 weight_v pv^2 * 2 v.a / v_max^2 + 3 weight_a pa^2 * 2 a.j / a_max^2]
 *   d_peak        [n_traj][2]: the largest sampled |v| / v_max and |a| / a_max of the trajectory
 * Each output may be NULL (all NULL: UAVQP_OK, nothing done).  For coefficients of uavqp_solve_batch_device at d_times, the TOTAL gradient
 * of Phi in the durations is
 *       d_grad_times + uavqp_solve_backward_device(g = d_grad_coeff).grad_times.
 *   d_status      [n_traj] status of the solve, or NULL (every trajectory counts as solved).  A trajectory whose status is not UAVQP_SOLVED,
 *                 or with M < 1, gets zeros everywhere.
 * Every output element is written exactly once, zeros included: no memset is needed beforehand.  The additions are in a fixed order: the
 * same bytes run to run and for any grid.  One launch, asynchronous on the ctx stream, no allocation, no read-back.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, samples_per_seg < 1, a limit or weight that is not finite, a
 * limit <= 0, a weight < 0, NULL times / coeff, ragged without offsets. */
typedef struct uavqp_limit_params {
    int32_t struct_size;
    int32_t samples_per_seg;   /* K: K + 1 sample points per segment (default 8) */
    double v_max;              /* speed limit, m/s (default 7: uavqp_default_pipeline_params) */
    double a_max;              /* acceleration limit, m/s^2 (default 10) */
    double weight_v;           /* >= 0 (default 1e3) */
    double weight_a;           /* >= 0 (default 1e3) */
} uavqp_limit_params;
void uavqp_default_limit_params(uavqp_limit_params* out);   /* callable without a device */
int uavqp_limit_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                               const double* d_coeff, const int32_t* d_status, const uavqp_limit_params* params, double* d_penalty,
                               double* d_grad_coeff, double* d_grad_times, double* d_peak);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_limit_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                             const double* coeff, const int32_t* status, const uavqp_limit_params* params, double* penalty,
                             double* grad_coeff, double* grad_times, double* peak);

/* uavqp_time_optimize_device with the limit penalty inside the objective: per trajectory
 *       minimise  f(T) = J(T) + time_weight * sum_i T_i + Phi(c*(T), T)     subject to  t_min <= T_i <= t_max.
 * c*(T) is still the minimiser of J alone (the QP does not see the penalty), so dJ/dT_i = -H_i still holds and
 *       df/dT_i = -H_i + time_weight + d_grad_times_i + uavqp_solve_backward_device(g = d_grad_coeff).grad_times_i
 * with the two penalty gradients above.  Method, parameters, Armijo rule, projection, arguments and outputs are those of
 * uavqp_time_optimize_device, f and its gradient replaced; host sequencing
 *       clamp, solve, [penalty, backward], step, max_iters x { solve at the trial durations, [penalty, backward], step }, solve
 * with every decision on the device, nothing read back, the number of launches depending on max_iters alone.  d_objective_out holds f
 * INCLUDING Phi; d_coeff_out is bit for bit uavqp_solve_batch_device at the durations handed back.  With weight_v = weight_a = 0, or limits
 * nothing reaches, every output equals that of uavqp_time_optimize_device byte for byte.
 *   limits       validated as for uavqp_limit_penalty_device
 *   d_peak_out   [n_traj][2] (may be NULL): sampled |v| / v_max and |a| / a_max at the durations handed back (zeros for a trajectory that is
 *                not UAVQP_SOLVED)
 * THE PENALTY IS SOFT: at finite weights the result may exceed the limits.  Expect sampled peaks a few per cent above a limit that binds (a
 * CPU simulation of this method at weight 1e3 left 3-12 % with limits set to 0.7 x the unconstrained peak).  The hard guarantee remains
 * uavqp_time_reallocate_device afterwards, which then has far less to stretch.
 * Out of scope: corridor and general-rows solves, multi-GPU (shard the batch as for the solve). */
int uavqp_time_optimize_limits_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                      const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                      const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out,
                                      double* d_objective_out, int32_t* d_accepted_out, const uavqp_limit_params* limits,
                                      double* d_peak_out);
/* The same from HOST pointers (as uavqp_time_optimize_host). */
int uavqp_time_optimize_limits_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                    const double* waypoints, double* times, const double* bc, const uavqp_time_opt_params* params,
                                    double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out,
                                    const uavqp_limit_params* limits, double* peak_out);

/* Signed Euclidean distance field of an occupancy grid, and the clearance penalty of solved trajectories against it.  Replaces, for one
 * map held on the device, plan_env/SDFMap: cloudCallback (src/planner/plan_env/src/sdf_map.cpp:836-927), updateESDF3d (:193-327) and
 * getDistWithGradTrilinear (include/plan_env/sdf_map.h:328-373).
 * A uavqp_esdf is opaque and owns its device buffers, all allocated by uavqp_esdf_create: nothing is allocated afterwards, every other
 * entry is asynchronous on the ctx stream and reads nothing back.  Grid: dims voxels of edge `resolution` from `origin`; arrays are
 * [nx][ny][nz], z fastest (the reference's toAddress).
 *   create     UAVQP_ERR_INVALID_ARG: a dimension below 1 or above 1024, more than 2^30 voxels, an origin that is not finite, resolution or
 *              max_dist not finite and positive.  The grid starts all free.  destroy synchronises the ctx stream first.
 *   set_occupancy_device   d_occ [nx][ny][nz] bytes: 0 free, non-zero occupied (stored as given).
 *   rasterize_cloud_device cloudCallback :858-906 without its camera window.  For every point p of d_obstacles [n_obs][3] and every integer
 *              (x, y, z) with |x|, |y| <= inflate_xy and |z| <= inflate_z: q = p + (x, y, z) * resolution in float64,
 *              id = floor((q - origin) * (1 / resolution)) per axis (the reference's posToIndex: a multiplication with the inverse); if all
 *              three indices lie inside the grid that voxel is set to 1.  The reference's values are inflate_xy =
 *              ceil(obstacles_inflation / resolution) and inflate_z = 1.  clear_first != 0 zeroes the grid before marking, 0 accumulates.
 *              Marking is idempotent (plain byte stores of 1): the result does not depend on the order of the points.
 *              UAVQP_ERR_INVALID_ARG: a negative inflation, one above 1024, a negative count.
 *   update_device   updateESDF3d over the whole grid.  sq_pos[v] = the exact integer squared voxel distance from v to the nearest occupied
 *              voxel, sq_neg[v] = the same to the nearest free voxel; both int32, INT32_MAX where no such voxel exists.
 *              d_pos = min(resolution * sqrt(sq_pos), max_dist), d_neg likewise; dist = d_pos if d_neg == 0, else d_pos - d_neg + resolution
 *              (:316-326).  max_dist stands in for the reference's unguarded "no obstacle" value (10000 is its buffer fill, :89-91).
 *              The integer fields are exactly the Euclidean transform (three separable passes in integers).
 *   read_device     copies of occupancy / sq_pos / sq_neg / dist into caller buffers of n voxels each; each may be NULL.
 *   query_device    getDistWithGradTrilinear for d_pts [n][3]: d_dist [n], d_grad [n][3], d_inside [n] bytes, each may be NULL.
 *              Outside the map (any axis < origin + 1e-4 or > origin + dims * resolution - 1e-4, or not a number): dist = 0, grad = 0,
 *              inside = 0.  Otherwise idx = floor((pos - 0.5 res - origin) / res), diff = (pos - ((idx + 0.5) res + origin)) / res (both
 *              divisions as multiplications with 1 / res), the eight values at idx + {0, 1}^3 with every index clamped into the grid
 *              (boundIndex), and the reference's interpolation and three gradient expressions (:355-370).  The gradient is discontinuous
 *              across the faces diff = 0.
 *   query_host      the same from HOST pointers (H2D copy, run, D2H copy, synchronous); the map stays a device object.
 * UAVQP_ERR_INVALID_ARG everywhere: a NULL esdf, a map of another device; query, penalty, and read of a field before the first update. */
typedef struct uavqp_esdf uavqp_esdf;
int uavqp_esdf_create(uavqp_ctx* ctx, const int32_t dims[3], const double origin[3], double resolution, double max_dist, uavqp_esdf** out);
int uavqp_esdf_destroy(uavqp_ctx* ctx, uavqp_esdf* esdf);
int uavqp_esdf_set_occupancy_device(uavqp_ctx* ctx, uavqp_esdf* esdf, const uint8_t* d_occ);
int uavqp_esdf_rasterize_cloud_device(uavqp_ctx* ctx, uavqp_esdf* esdf, const double* d_obstacles, int n_obs, int inflate_xy, int inflate_z,
                                      int clear_first);
int uavqp_esdf_update_device(uavqp_ctx* ctx, uavqp_esdf* esdf);
int uavqp_esdf_read_device(uavqp_ctx* ctx, uavqp_esdf* esdf, uint8_t* d_occ, int32_t* d_sq_pos, int32_t* d_sq_neg, double* d_dist);
int uavqp_esdf_query_device(uavqp_ctx* ctx, uavqp_esdf* esdf, int n_pts, const double* d_pts, double* d_dist, double* d_grad,
                            uint8_t* d_inside);
int uavqp_esdf_query_host(uavqp_ctx* ctx, uavqp_esdf* esdf, int n_pts, const double* pts, double* dist, double* grad, uint8_t* inside);

/* Clearance penalty of solved trajectories against a distance field, with its gradients: the shape of uavqp_limit_penalty_device.  Per
 * trajectory, K = samples_per_seg, tau_s = s / K, trapezoid weights om_0 = om_K = 1/2, om_s = 1 otherwise, pos(x) = max(0, x),
 * p = p_i(tau_s T_i) the 3-axis position of segment i, d(p) and grad d the field query above:
 *   Phi = sum_i (T_i / K) sum_{s=0..K} om_s * weight * pos((d_safe - d(p)) / d_safe)^3        over the samples inside the map
 * A sample outside the map contributes nothing and is counted in d_outside.  With e = -3 weight pos(.)^2 / d_safe:
 *   d_penalty     [n_traj] Phi
 *   d_grad_coeff  layout and basis of coeff ([axis][segment][2r] per trajectory): dPhi/dc at FIXED durations,
 *                 (T_i / K) om_s e * grad d[axis] * dp/dc per sample (dp/dc_k = t^k)
 *   d_grad_times  [sum_b M_b]: the EXPLICIT dPhi/dT_i at FIXED coefficients, Phi_i / T_i + (T_i / K) sum_s om_s tau_s e (grad d . v), v the
 *                 velocity of the sample
 *   d_min_dist    [n_traj] the smallest sampled distance inside the map (max_dist of the map if no sample is inside)
 *   d_outside     [n_traj] int32 samples outside the map
 * Each output may be NULL (all NULL: UAVQP_OK, nothing done).  For coefficients of uavqp_solve_batch_device at d_times, the TOTAL gradient
 * of Phi in the durations is
 *       d_grad_times + uavqp_solve_backward_device(g = d_grad_coeff).grad_times,
 * and grad_waypoints / grad_bc of that same call are the gradients in the waypoints and boundary conditions.
 *   d_status      [n_traj] status of the solve, or NULL (every trajectory counts as solved).  A trajectory whose status is not UAVQP_SOLVED,
 *                 or with M < 1, gets zeros (min_dist = max_dist, outside = 0).
 * Every output element is written exactly once, zeros included.  The additions are in a fixed order: the same bytes run to run and for
 * any grid.  One launch, asynchronous on the ctx stream, no allocation, no read-back.  The penalty is piecewise smooth: its gradients
 * jump where a sample crosses a cell face of the trilinear query or a bound of the map (at d = d_safe the cube keeps them continuous).
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, samples_per_seg < 1, d_safe not finite or <= 0, weight not
 * finite or < 0, a NULL esdf or one never updated, NULL times / coeff, ragged without offsets.
 * An optimiser over the waypoints that uses the penalty: uavqp_waypoint_optimize_device below; over waypoints AND durations, together with
 * the limit penalty: uavqp_spacetime_optimize_device.
 * Out of scope: local-window updates, batches of maps, multi-GPU. */
typedef struct uavqp_clearance_params {
    int32_t struct_size;
    int32_t samples_per_seg;   /* K: K + 1 sample points per segment (default 8) */
    double d_safe;             /* clearance below which a sample is penalised, m (default 0.5) */
    double weight;             /* >= 0 (default 1e3) */
} uavqp_clearance_params;
void uavqp_default_clearance_params(uavqp_clearance_params* out);   /* callable without a device */
int uavqp_clearance_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                                   const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf,
                                   const uavqp_clearance_params* params, double* d_penalty, double* d_grad_coeff, double* d_grad_times,
                                   double* d_min_dist, int32_t* d_outside);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous); esdf stays a device object. */
int uavqp_clearance_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                 const double* coeff, const int32_t* status, const uavqp_esdf* esdf, const uavqp_clearance_params* params,
                                 double* penalty, double* grad_coeff, double* grad_times, double* min_dist, int32_t* outside);

/* EXACT gradient of the control cost with respect to the waypoints: the counterpart of uavqp_cost_time_gradient_device (no reference
 * counterpart).  Per trajectory, from the coefficients a solve wrote, in WAYPOINT layout -- all M_b + 1 knots, both ends included:
 *   grad[seg_offsets[b] + b + k][axis] = dJ_b / dp_k = 2 (-1)^(r-1) (2r-1)! (c_{k-1,2r-1} - c_{k,2r-1})
 * c_{i,2r-1} the leading coefficient of segment i on that axis; at k = 0 only the second term, at k = M only the first.  r = 3:
 * 240 (c_{k-1,5} - c_{k,5}); r = 4: -10080 (c_{k-1,7} - c_{k,7}).  (r integrations by parts of the variation of J; the terms in the knot
 * derivatives vanish at the minimiser -- free and stationary at an interior knot, fixed at an end --, p^(2r) = 0 inside a segment and
 * p^(2r-1) is constant along it.)  The end rows are the derivatives with respect to the end POSITIONS at fixed boundary derivatives.
 * The gradient is that of the OPTIMAL cost: meaningful for coefficients of uavqp_solve_batch_* (corridor and general-rows solves are out
 * of scope).  It equals uavqp_solve_backward_device(g = 2 P c).grad_waypoints up to rounding, without a factorisation.  The durations do
 * not enter, so there is no d_times argument.
 *   d_status  [n_traj] status of the solve, or NULL (every trajectory counts as solved).  A trajectory whose status is not UAVQP_SOLVED, or
 *             with M < 1, gets zeros.
 *   d_grad    [sum_b (M_b + 1)][3]; NULL: UAVQP_OK, nothing done.  Every element is written exactly once.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, NULL coeff, ragged without offsets.  One launch, asynchronous on the ctx stream, no
 * allocation, no read-back. */
int uavqp_cost_waypoint_gradient_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                        const double* d_coeff, const int32_t* d_status, double* d_grad);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_cost_waypoint_gradient_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                      const double* coeff, const int32_t* status, double* grad);

/* Optimisation of the INTERIOR WAYPOINTS against a distance field: a gradient-based planner back-end in the style of GCOPTER / EGO-Planner
 * (no reference counterpart: the reference never moves a searched waypoint).  Per trajectory, with the durations, the boundary derivatives
 * and both end waypoints fixed,
 *       minimise over p_1 .. p_{M-1}   f(p) = smooth_weight * J(p) + Phi(c*(p), T)
 *       subject to                     |p_k[axis] - p_k^start[axis]| <= max_move      for every interior knot and axis
 * J the control cost at the minimiser c*(p) of the equality-constrained QP, Phi exactly the penalty of uavqp_clearance_penalty_device
 * against `esdf`.  c*(p) stays the minimiser of J alone (the QP does not see the penalty), so
 *       df/dp_k = smooth_weight * uavqp_cost_waypoint_gradient_device_k + uavqp_solve_backward_device(g = dPhi/dc).grad_waypoints_k.
 * Method (that of uavqp_time_optimize_device): projected gradient descent with Armijo backtracking along the projection arc.  Direction
 * d_k = (df/dp_k) / s_k with the per-knot scale s_k = T_{k-1}^-(2r-1) + T_k^-(2r-1) > 0 (J scales like T^-(2r-1): one step length then
 * serves knots between short and between long segments; -d is still a descent direction), a component zero where the box blocks it.
 * The first alpha makes the largest |alpha d| equal to initial_step metres.  A trial p - alpha d, clamped into the box, is accepted iff its
 * solve ends UAVQP_SOLVED and f_trial <= f - armijo_c * sum_k (df/dp_k) . (p_k - p_trial_k); accepted: alpha *= grow, rejected:
 * alpha *= shrink.  f never increases.  A trajectory without a direction at the start (no interior knot, or a gradient that is zero in
 * every component the box leaves free) proposes nothing and accepts nothing.
 * Host-side C++ sequencing of
 *       anchor copy, solve, penalty, backward, step, max_iters x { solve at the trial waypoints, penalty, backward, step }, solve, penalty
 * (the last penalty only for d_min_dist_out / d_outside_out): every accept / reject is taken per trajectory ON THE DEVICE, nothing is read
 * back, the number of launches depends on max_iters alone.  The additions are in a fixed order: the same bytes run to run and for any
 * grid.  Asynchronous on the ctx stream (a first call of a given size allocates the workspace).
 *   d_waypoints      [sum_b (M_b + 1)][3] IN: the start, OUT: the accepted waypoints.  The two end knots of every trajectory come back byte
 *                    for byte; so does every knot of a trajectory that is not UAVQP_SOLVED at the start (e.g. a non-positive duration:
 *                    UAVQP_INVALID_INPUT) -- it keeps its status and takes no part.
 *   d_times, d_bc    as for uavqp_solve_batch_device; not changed
 *   esdf, clearance  validated as for uavqp_clearance_penalty_device
 *   d_coeff_out      the solve AT the waypoints handed back: bit for bit what uavqp_solve_batch_device writes for them
 *   d_status_out     [n_traj] status of that solve (may be NULL)
 *   d_objective_out  [n_traj][2]: f at the start, f at the result (NaN, NaN for a trajectory that took no part)
 *   d_accepted_out   [n_traj] int32 accepted trials (may be NULL)
 *   d_min_dist_out   [n_traj], d_outside_out [n_traj] int32: the penalty's two diagnostics at the result (each may be NULL)
 *   params           uavqp_default_waypoint_opt_params fills the defaults; UAVQP_ERR_INVALID_ARG for a wrong struct_size, max_iters < 0,
 *                    smooth_weight < 0, max_move <= 0 (INFINITY is allowed: no box), initial_step <= 0, armijo_c outside (0, 1), shrink
 *                    outside (0, 1), grow < 1 or any other non-finite value.  max_iters = 0: the plain solve, both objective columns equal,
 *                    the waypoints untouched.
 * UAVQP_ERR_INVALID_ARG also: r not 3 / 4, a negative count, a NULL esdf or one never updated, invalid clearance parameters, a NULL
 * waypoints / times / bc / coeff_out / objective_out, ragged without offsets or with max_segments < 1, uniform with total_segments !=
 * uniform_segments * n_traj.
 * WHAT THE RESULT IS.  A sample outside the map contributes nothing to Phi, so f JUMPS DOWN where a sample leaves the map: max_move is the
 * caller's handle to keep the trajectories inside (check d_outside_out).  The penalty is piecewise smooth (its gradient jumps across the
 * cell faces of the trilinear query), so the method converges to a point where no descent step of the tried lengths is left, not to a
 * stationary point in the classical sense.  The result is a LOCAL minimum of a SOFT penalty: at finite weight a trajectory may end closer
 * than d_safe, and a start on the symmetric saddle of an obstacle (gradient zero) does not move.  uavqp_ellipsoid_check_* afterwards
 * remains the hard test.
 * Joint optimisation of the durations: uavqp_spacetime_optimize_device below.
 * Out of scope: corridor and general-rows solves, multi-GPU (shard the batch as for the solve: trajectories are independent). */
typedef struct uavqp_waypoint_opt_params {
    int32_t struct_size;
    int32_t max_iters;      /* trials per trajectory (default 64) */
    double smooth_weight;   /* weight of the control cost J, >= 0 (default 1) */
    double max_move;        /* half edge of the box around every start waypoint, m, > 0, may be INFINITY (default 2) */
    double initial_step;    /* largest move of a waypoint component in the first trial, m (default 0.1) */
    double armijo_c;        /* sufficient-decrease constant (default 1e-4) */
    double shrink;          /* step factor after a rejected trial (default 0.5) */
    double grow;            /* ... after an accepted one (default 2) */
} uavqp_waypoint_opt_params;
void uavqp_default_waypoint_opt_params(uavqp_waypoint_opt_params* out);   /* callable without a device */
int uavqp_waypoint_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                   const int32_t* d_seg_offsets, double* d_waypoints, const double* d_times, const double* d_bc,
                                   const uavqp_esdf* esdf, const uavqp_clearance_params* clearance, const uavqp_waypoint_opt_params* params,
                                   double* d_coeff_out, int32_t* d_status_out, double* d_objective_out, int32_t* d_accepted_out,
                                   double* d_min_dist_out, int32_t* d_outside_out);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous; waypoints is updated in place; the map stays a device object; the
 * coefficients of a trajectory that is not UAVQP_SOLVED come back as they do from uavqp_solve_batch_host). */
int uavqp_waypoint_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                 double* waypoints, const double* times, const double* bc, const uavqp_esdf* esdf,
                                 const uavqp_clearance_params* clearance, const uavqp_waypoint_opt_params* params, double* coeff_out,
                                 int32_t* status_out, double* objective_out, int32_t* accepted_out, double* min_dist_out, int32_t* outside_out);

/* Fused flight penalty: the limit penalty and the clearance penalty of solved trajectories in ONE launch (the hot path of
 * uavqp_spacetime_optimize_device below).  Per trajectory
 *       Phi = Phi_lim + Phi_clr
 * Phi_lim exactly the formula of uavqp_limit_penalty_device with `limits`, Phi_clr exactly that of uavqp_clearance_penalty_device with
 * `clearance` against `esdf`; each part keeps its own samples_per_seg.
 *   d_penalty     [n_traj] Phi
 *   d_grad_coeff  layout of coeff ([axis][segment][2r] per trajectory): dPhi/dc at FIXED durations, the sum of both parts
 *   d_grad_times  [sum_b M_b]: the EXPLICIT dPhi/dT_i at FIXED coefficients, the sum of both parts
 *   d_peak        [n_traj][2] as uavqp_limit_penalty_device writes it
 *   d_min_dist    [n_traj], d_outside [n_traj] int32 as uavqp_clearance_penalty_device writes them
 * Each output may be NULL (all NULL: UAVQP_OK, nothing done).  The TOTAL gradients of Phi in the durations and in the waypoints come out of
 * one uavqp_solve_backward_device(g = d_grad_coeff): d_grad_times + its grad_times, and its grad_waypoints.
 * A lane loads the coefficients and the duration of a segment once and runs both sets of samples over them.  With weight_v = weight_a = 0
 * the limit part contributes nothing, with clearance weight 0 the clearance part contributes nothing (the diagnostics of a part are
 * still those of its own entry).  d_status, unsolved trajectories and M < 1 as for the two entries: zeros, min_dist = max_dist.
 * Every output element is written exactly once, zeros included.  The additions are in a fixed order: the same bytes run to run and for
 * any grid.  One launch, asynchronous on the ctx stream, no allocation, no read-back.  Piecewise smooth, as the clearance penalty is.
 * UAVQP_ERR_INVALID_ARG: whatever either of the two entries refuses. */
int uavqp_flight_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                                const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                const uavqp_clearance_params* clearance, double* d_penalty, double* d_grad_coeff, double* d_grad_times,
                                double* d_peak, double* d_min_dist, int32_t* d_outside);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous); esdf stays a device object. */
int uavqp_flight_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                              const double* coeff, const int32_t* status, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                              const uavqp_clearance_params* clearance, double* penalty, double* grad_coeff, double* grad_times, double* peak,
                              double* min_dist, int32_t* outside);

/* JOINT optimisation of the interior waypoints and the durations under both penalties: what a GCOPTER / MINCO-style back-end gives -- a
 * trajectory that is smooth, short in time, within v_max / a_max and clear of obstacles -- as one call (no reference counterpart).  Per
 * trajectory, with the boundary derivatives and both end waypoints fixed,
 *       minimise over p_1 .. p_{M-1}, T_0 .. T_{M-1}   f(p, T) = smooth_weight * J + time_weight * sum_i T_i + Phi(c*(p, T), T)
 *       subject to   |p_k[axis] - p_k^start[axis]| <= max_move,   t_min <= T_i <= t_max
 * J the control cost at the minimiser c*(p, T) of the equality-constrained QP (the QP does not see the penalty), Phi the fused flight
 * penalty above.  Gradients, all from entries above:
 *       df/dp_k = smooth_weight * uavqp_cost_waypoint_gradient_device_k + uavqp_solve_backward_device(g = dPhi/dc).grad_waypoints_k
 *       df/dT_i = -smooth_weight * H_i + time_weight + (explicit dPhi/dT_i) + uavqp_solve_backward_device(g = dPhi/dc).grad_times_i
 * (H_i: uavqp_cost_time_gradient_device; one backward call gives both backward terms.)
 * Method (that of uavqp_waypoint_optimize_device and uavqp_time_optimize_device, joined): projected gradient descent with Armijo
 * backtracking along the projection arc, in p and in u_i = log T_i.  Directions: d^p_k = (df/dp_k) / s_k, s_k = T_{k-1}^-(2r-1) + T_k^-(2r-1)
 * at the current best durations, a component zero where the box blocks it; d^u_i = T_i df/dT_i, zero where a bound blocks it.  The two
 * blocks have different units, so each gets a scale fixed at the start: sigma_p = initial_step_move / max |d^p|, sigma_u =
 * initial_step_log / max |d^u| (a scale is 0 when its maximum is 0 or not finite); alpha starts at 1, or at 0 if both scales are 0 (such a
 * trajectory proposes nothing and accepts nothing).  A positive diagonal scaling keeps -(sigma_p d^p, sigma_u d^u) a descent direction.
 * Trial: p_t = clamp(p - alpha sigma_p d^p), T_t = clamp(T exp(-alpha sigma_u d^u)); accepted iff alpha > 0, its solve ends UAVQP_SOLVED
 * and  f_trial <= f - armijo_c * [ sum_k (df/dp_k) . (p_k - p_t,k) + sum_i d^u_i log(T_i / T_t,i) ];  accepted: alpha *= grow, rejected:
 * alpha *= shrink.  ONE accept / reject per trajectory and trial; f never increases.  A trajectory with M = 1 takes part through its duration alone.
 * Host-side C++ sequencing of
 *       anchor copy, clamp, solve, flight penalty, backward, step,
 *       max_iters x { solve at the trial waypoints and durations, flight penalty, backward, step }, solve, flight penalty
 * (the last penalty only for the three diagnostics): four launches per iteration, every decision ON THE DEVICE, nothing read back, the
 * number of launches depends on max_iters alone.  The additions are in a fixed order: the same bytes run to run and for any grid.
 * Asynchronous on the ctx stream (a first call of a given size allocates the workspace).
 *   d_waypoints      [sum_b (M_b + 1)][3] IN: the start, OUT: the accepted waypoints; the two end knots come back byte for byte
 *   d_times          [sum_b M_b] IN: the start, OUT: the accepted durations.  Durations of a trajectory that are all positive and finite
 *                    are first projected into [t_min, t_max] (as uavqp_time_optimize_device does)
 *                    A trajectory that is not UAVQP_SOLVED at the start (e.g. a non-positive duration: UAVQP_INVALID_INPUT) keeps its status,
 *                    waypoints and durations byte for byte and takes no part -- except that the projection above comes before the first
 *                    solve: a trajectory with all-positive, finite durations that fails to solve for another reason (a waypoint that
 *                    is not finite) comes back with its durations projected, as from uavqp_time_optimize_device.
 *   d_bc             as for uavqp_solve_batch_device; not changed
 *   esdf, limits, clearance   validated as for uavqp_flight_penalty_device
 *   d_coeff_out      the solve AT what is handed back: bit for bit what uavqp_solve_batch_device writes for it; d_status_out [n_traj] its
 *                    status (may be NULL)
 *   d_objective_out  [n_traj][2]: f at the start (after the projection of the durations), f at the result (NaN, NaN: took no part)
 *   d_accepted_out   [n_traj] int32 accepted trials (may be NULL)
 *   d_peak_out [n_traj][2], d_min_dist_out [n_traj], d_outside_out [n_traj] int32: the penalty's diagnostics at the result (each may be NULL)
 *   params           uavqp_default_spacetime_params fills the defaults (those of the two optimisers it joins; max_iters from the CPU study of
 *                    DESIGN.md section 5.20).  UAVQP_ERR_INVALID_ARG for a wrong struct_size, max_iters < 0 or > 100000, smooth_weight < 0,
 *                    time_weight <= 0, t_min <= 0, t_min > t_max, max_move <= 0 (INFINITY is allowed: no box), an initial step <= 0,
 *                    armijo_c outside (0, 1), shrink outside (0, 1), grow < 1 or any other non-finite value.  max_iters = 0: the plain
 *                    solve, both objective columns equal, waypoints and durations untouched apart from the projection.
 * UAVQP_ERR_INVALID_ARG also: r not 3 / 4, a negative count, NULL waypoints / times / bc / coeff_out / objective_out, ragged without offsets
 * or with max_segments < 1, uniform with total_segments != uniform_segments * n_traj.
 * WHAT THE RESULT IS.  Both penalties are SOFT: at finite weights the result may exceed a limit by a few per cent and may end closer than
 * d_safe.  A sample outside the map contributes nothing to the clearance part, so f JUMPS DOWN where a sample leaves the map: max_move is
 * the caller's handle (check d_outside_out).  The clearance part is piecewise smooth (its gradient jumps across the cell faces of the
 * trilinear query), so the method converges to a point where no descent step of the tried lengths is left; the result is a LOCAL minimum,
 * and a start on the symmetric saddle of an obstacle does not move sideways.  The two scales are fixed at the FIRST gradient: from a start far
 * outside the limits (a gradient of 1e7 in the durations) the duration block moves slowly once the penalty has gone, and alternating
 * uavqp_time_optimize_limits_device with uavqp_waypoint_optimize_device, which re-scales at every call, ended lower with the same number of
 * solves; a second call of this entry re-scales too.  The hard tests remain uavqp_time_reallocate_device (limits: it
 * then has far less to stretch) and uavqp_ellipsoid_check_* (collisions).
 * Out of scope: corridor and general-rows solves, capture into a graph, multi-GPU (shard the batch as for the solve).  Quasi-Newton
 * directions: uavqp_spacetime_lbfgs_device below. */
typedef struct uavqp_spacetime_params {
    int32_t struct_size;
    int32_t max_iters;          /* trials per trajectory (default 32) */ 
    double smooth_weight;       /* weight of the control cost J, >= 0 (default 1) */
    double time_weight;         /* weight of the total duration, > 0 (default 50) */
    double t_min;               /* bounds of every duration, s (defaults 1e-2, 1e2) */
    double t_max;
    double max_move;            /* half edge of the box around every start waypoint, m, > 0, may be INFINITY (default 2) */
    double initial_step_move;   /* largest move of a waypoint component in the first trial, m (default 0.1) */
    double initial_step_log;    /* largest change of log T_i in the first trial (default 0.1) */
    double armijo_c;            /* sufficient-decrease constant (default 1e-4) */
    double shrink;              /* step factor after a rejected trial (default 0.5) */
    double grow;                /* ... after an accepted one (default 2) */
} uavqp_spacetime_params;
void uavqp_default_spacetime_params(uavqp_spacetime_params* out);   /* callable without a device */
int uavqp_spacetime_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                    const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                    const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                    const uavqp_spacetime_params* params, double* d_coeff_out, int32_t* d_status_out, double* d_objective_out,
                                    int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out, int32_t* d_outside_out);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous; waypoints and times are updated in place; the map stays a device
 * object; the coefficients of a trajectory that is not UAVQP_SOLVED come back as they do from uavqp_solve_batch_host). */
int uavqp_spacetime_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                  double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                  const uavqp_clearance_params* clearance, const uavqp_spacetime_params* params, double* coeff_out,
                                  int32_t* status_out, double* objective_out, int32_t* accepted_out, double* peak_out, double* min_dist_out,
                                  int32_t* outside_out);

/* The same joint optimisation with LIMITED-MEMORY BFGS directions, kept per trajectory on the device: the objective f, the variables, the
 * bounds, the gradients, every argument and output, the projection of the durations before the first solve, the treatment of trajectories
 * that are not UAVQP_SOLVED at the start or have M = 1, the meaning of d_objective_out / d_accepted_out / d_peak_out / d_min_dist_out /
 * d_outside_out and the rule "d_coeff_out is bit for bit the plain solve at what is handed back" are those of
 * uavqp_spacetime_optimize_device above.  Only the direction of a trial differs.  Per trajectory:
 * Variables.  x = (p_k[axis] / initial_step_move for the interior knots k, log T_i / initial_step_log): the units in which the first step
 * of either block has length one.  g = (initial_step_move df/dp_k[axis], initial_step_log T_i df/dT_i), df/dp and df/dT as above.  lo, hi:
 * the box and [log t_min, log t_max] in these units.  The device keeps p and T themselves: a trial is formed as
 *       p_t = clamp(p + alpha initial_step_move d^p),  T_t = clamp(T exp(alpha initial_step_log d^u))            (d in x)
 * and x_t - x = ((p_t - p) / initial_step_move, log(T_t / T) / initial_step_log), so a component whose d is zero keeps its bytes.
 * Free set at the best point: component i is BLOCKED when x_i <= lo_i and g_i > 0, or x_i >= hi_i and g_i < 0.
 * Gradient mode (at the start, and after every reset).  The direction of uavqp_spacetime_optimize_device: d^p_k = (df/dp_k) / s_k, d^u_i =
 * T_i df/dT_i, blocked components zero; sigma_p = initial_step_move / max |d^p|, sigma_u = initial_step_log / max |d^u| (0 when the
 * maximum is 0 or not finite), computed AT THE CURRENT BEST POINT EVERY TIME THE MODE IS ENTERED; alpha = 1 on entry (0 when both scales
 * are 0).  Trial: p_t = clamp(p - alpha sigma_p d^p), T_t = clamp(T exp(-alpha sigma_u d^u)), the directions taken at the best point.
 * Accepted: alpha *= grow, rejected: alpha *= shrink.  With max_iters = 1 every output is that of uavqp_spacetime_optimize_device.
 * Quasi-Newton mode (whenever at least one pair is stored, after an accepted trial).  The two-loop recursion over the stored pairs (s_j,
 * y_j), newest to oldest and back, started at q = g; the blocked components of g, s_j and y_j count as zero in every dot product and
 * every update; a pair whose masked s_j . y_j is not positive is skipped; H0 = gamma I with gamma = s . y / y . y of the NEWEST pair,
 * masked the same way.  d = minus the result, blocked components zero; alpha = 1 for every new direction.  If gamma is not positive and
 * finite, or unless g_F . d < -1e-10 |g_F| |d| (g_F: g with its blocked components zero), the memory is cleared and gradient mode is
 * entered at this point.
 * Trial: accepted iff alpha > 0, its solve ends UAVQP_SOLVED and  f_t <= f - armijo_c * g . (x - x_t), i.e.
 *       f_t <= f - armijo_c * [ sum_k (df/dp_k) . (p_k - p_t,k) + sum_i T_i (df/dT_i) log(T_i / T_t,i) ]
 * (the rule of uavqp_spacetime_optimize_device in these units).  ONE accept / reject per trajectory and trial; f never increases.
 * Accepted: s = x_t - x, y = g_t - g (NOT masked); the pair is stored iff s . y > curvature_eps |s| |y|; the memory holds the `memory`
 * newest pairs.  The next direction is quasi-Newton if the memory is not empty; otherwise gradient mode goes on (alpha *= grow, the
 * scales stay).
 * Rejected: alpha *= shrink, the direction stays.  In quasi-Newton mode, after max_backtracks consecutive rejections the memory is cleared
 * and gradient mode is entered at the best point.
 * Sequencing, cost per trial (four launches), determinism and asynchrony as above; the history (memory + 1 slots of s and y per
 * trajectory) lives in the workspace the first call of a given size allocates.
 *   params   uavqp_default_spacetime_lbfgs_params fills the defaults: max_iters 32, memory 8, max_backtracks 6, curvature_eps 1e-10
 *            (DESIGN.md section 5.21), every other field as uavqp_default_spacetime_params.  UAVQP_ERR_INVALID_ARG for a wrong
 *            struct_size, whatever uavqp_spacetime_optimize_device refuses in a field of the same name, memory outside 1 .. 16,
 *            max_backtracks outside 1 .. 64, curvature_eps outside [0, 1) or not a number.
 * WHAT THE RESULT IS: as above, a local minimum of a piecewise smooth f with soft penalties.  On the test batches 32 trials leave 1e-3 of
 * the decrease scipy's L-BFGS-B reaches, against 2e-2 for uavqp_spacetime_optimize_device.
 * Out of scope: a Wolfe line search (one trial per iteration keeps the launch count fixed), corridor and general-rows solves, capture into
 * a graph, multi-GPU (shard the batch as for the solve). */
typedef struct uavqp_spacetime_lbfgs_params {
    int32_t struct_size;
    int32_t max_iters;          /* trials per trajectory (default 32) */
    int32_t memory;             /* stored pairs per trajectory, 1 .. 16 (default 8) */
    int32_t max_backtracks;     /* consecutive rejections of a quasi-Newton direction before the memory is cleared, 1 .. 64 (default 6) */
    double smooth_weight;       /* the fields of uavqp_spacetime_params, same meaning, defaults and validity */
    double time_weight;
    double t_min;
    double t_max;
    double max_move;
    double initial_step_move;   /* also the unit of the waypoint variables */
    double initial_step_log;    /* also the unit of the log-duration variables */
    double armijo_c;
    double shrink;
    double grow;                /* (gradient mode only) */
    double curvature_eps;       /* a pair is stored iff s . y > curvature_eps |s| |y|, in [0, 1) (default 1e-10) */
} uavqp_spacetime_lbfgs_params;
void uavqp_default_spacetime_lbfgs_params(uavqp_spacetime_lbfgs_params* out);   /* callable without a device */
int uavqp_spacetime_lbfgs_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                 const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                 const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                 const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out, int32_t* d_status_out,
                                 double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out,
                                 int32_t* d_outside_out);
/* The same from HOST pointers, as uavqp_spacetime_optimize_host. */
int uavqp_spacetime_lbfgs_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                               double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                               const uavqp_clearance_params* clearance, const uavqp_spacetime_lbfgs_params* params, double* coeff_out,
                               int32_t* status_out, double* objective_out, int32_t* accepted_out, double* peak_out, double* min_dist_out,
                               int32_t* outside_out);

/* Attitude penalty of solved trajectories with its gradients: what a multirotor must do to fly them -- how hard its rotors push, how far
 * it tilts, how fast its body turns (no reference counterpart as a penalty: the reference's so3_control derives attitude and thrust from
 * the commanded acceleration in the same way; the term is that of GCOPTER / MINCO, in a division-free form).  The shape of
 * uavqp_limit_penalty_device.  Per sample at segment-local time t let a, j, s be the acceleration, jerk and snap of the three axes,
 * z = a + gravity e_z the specific thrust vector (thrust per unit of mass, m/s^2), f2 = |z|^2.  With pos(x) = max(0, x) and
 * kappa = tan^2(tilt_max):
 *   u_hi   = f2 / f_max^2 - 1
 *   u_lo   = 1 - f2 / f_min^2                                                    (absent when f_min = 0)
 *   u_tilt = (z_x^2 + z_y^2 - kappa z_z |z_z|) / gravity^2
 *   u_rate = (|z x j|^2 - rate_max^2 f2^2) / (rate_max^2 gravity^4),             |z x j|^2 = f2 |j|^2 - (z.j)^2
 *   phi    = weight_thrust (pos(u_hi)^3 + pos(u_lo)^3) + weight_tilt pos(u_tilt)^3 + weight_rate pos(u_rate)^3
 *   Phi    = sum_i (T_i / K) sum_{s=0..K} om_s phi(tau_s T_i)
 * K = samples_per_seg, tau_s = s / K and the trapezoid weights om_s those of uavqp_limit_penalty_device.  The feasible sets are the
 * physical ones: u_hi <= 0 and u_lo <= 0 mean f_min <= |z| <= f_max; u_tilt <= 0 means a tilt of at most tilt_max with upward thrust
 * (thrust pointing below the horizon is penalised whatever tilt_max is); u_rate <= 0 means |b3 x db3/dt| = |z x j| / f2 <= rate_max, b3
 * the thrust axis.  NO term divides by |z|: every output is finite for every finite input, free fall (z = 0) costs exactly weight_thrust
 * per unit of weight (when f_min > 0) and has zero gradient.  Every u is dimensionless, so Phi has the unit of time_weight * T like the
 * other penalties, and the cube makes it twice continuously differentiable.  The yaw rate is NOT part of the body rate: these
 * trajectories carry no heading, the rate bounded is that of the thrust axis alone.
 * Gradients, G_a and G_j the derivatives of phi in a and j:
 *   G_a = 3 weight_thrust (pos(u_hi)^2 2 z / f_max^2 - pos(u_lo)^2 2 z / f_min^2)
 *       + 3 weight_tilt pos(u_tilt)^2 (2 z_x, 2 z_y, -2 kappa |z_z|) / gravity^2
 *       + 3 weight_rate pos(u_rate)^2 (2 |j|^2 z - 2 (z.j) j - 4 rate_max^2 f2 z) / (rate_max^2 gravity^4)
 *   G_j = 3 weight_rate pos(u_rate)^2 (2 f2 j - 2 (z.j) z) / (rate_max^2 gravity^4)
 *   d_penalty     [n_traj] Phi
 *   d_grad_coeff  layout of coeff: dPhi/dc_{axis,k} = (T_i / K) sum_s om_s [G_a[axis] k(k-1) t^(k-2) + G_j[axis] k(k-1)(k-2) t^(k-3)], at FIXED
 *                 durations
 *   d_grad_times  [sum_b M_b]: the EXPLICIT dPhi/dT_i = Phi_i / T_i + (T_i / K) sum_s om_s tau_s [G_a . j + G_j . s], at FIXED coefficients
 *   d_peak        [n_traj][4], in physical units, over the samples: the largest |z|, the smallest |z| (m/s^2), the largest tilt angle
 *                 atan2(sqrt(z_x^2 + z_y^2), z_z) (rad), the largest body rate |z x j| / f2 (rad/s; a sample with f2 = 0 is left out).  A
 *                 trajectory without a sample (not UAVQP_SOLVED, or M < 1) reports {0, +inf, 0, 0}.
 * Each output may be NULL (all NULL: UAVQP_OK, nothing done).  The TOTAL gradients in durations, waypoints and boundary derivatives of
 * coefficients that come from uavqp_solve_batch_device are d_grad_times + uavqp_solve_backward_device(g = d_grad_coeff), as for the other
 * penalties.  d_status as for uavqp_limit_penalty_device: a trajectory that is not UAVQP_SOLVED, or with M < 1, gets zeros in the penalty
 * and both gradients.  Every output element is written exactly once, zeros included; the additions are in a fixed order: the same bytes
 * run to run and for any grid.  One launch, asynchronous on the ctx stream, no allocation, no read-back.
 * WHAT THE RESULT IS: a SOFT penalty.  At finite weights a trajectory optimised against it may still exceed a limit that binds; d_peak is
 * the check afterwards, in the units of the limits themselves.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, samples_per_seg < 1, gravity not positive and finite, not
 * 0 <= f_min < f_max < inf, tilt_max outside (0, pi/2), rate_max not positive and finite, a weight that is negative or not finite, NULL
 * times / coeff, ragged without offsets. */
typedef struct uavqp_attitude_params {
    int32_t struct_size;
    int32_t samples_per_seg;   /* K: K + 1 sample points per segment (default 8) */
    double gravity;            /* m/s^2, > 0 (default 9.81, the constant the collision check's body frame uses) */
    double f_min;              /* smallest specific thrust, m/s^2, >= 0; 0: no lower limit (default 3) */
    double f_max;              /* largest specific thrust, m/s^2, > f_min (default 20: about twice the weight) */
    double tilt_max;           /* largest tilt of the thrust axis from vertical, rad, in (0, pi/2) (default 1.05) */
    double rate_max;           /* largest rate of the thrust axis, rad/s, > 0 (default 2.1) */
    double weight_thrust;      /* >= 0 (default 1e3) */
    double weight_tilt;        /* >= 0 (default 1e3) */
    double weight_rate;        /* >= 0 (default 1e3) */
} uavqp_attitude_params;
void uavqp_default_attitude_params(uavqp_attitude_params* out);   /* callable without a device */
int uavqp_attitude_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                  const double* d_times, const double* d_coeff, const int32_t* d_status,
                                  const uavqp_attitude_params* params, double* d_penalty, double* d_grad_coeff, double* d_grad_times,
                                  double* d_peak);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_attitude_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                const double* coeff, const int32_t* status, const uavqp_attitude_params* params, double* penalty,
                                double* grad_coeff, double* grad_times, double* peak);

/* uavqp_spacetime_lbfgs_device with the attitude penalty inside the objective: per trajectory
 *       minimise  f(p, T) = [the objective of uavqp_spacetime_lbfgs_device] + Phi_att(c*(p, T), T)
 * Phi_att exactly the formula of uavqp_attitude_penalty_device with `attitude`.  Variables, bounds, directions, the ONE accept / reject per
 * trajectory and trial, every argument, every output and the parameters are those of uavqp_spacetime_lbfgs_device; only f and its
 * gradient differ.  Sequencing: that of uavqp_spacetime_lbfgs_device with one more launch after every flight penalty that feeds a step
 * (the attitude penalty ADDS its value and both partial gradients to the flight penalty's before the one backward pass): five launches per
 * trial, still none that depends on the data, nothing read back.  d_objective_out holds f INCLUDING Phi_att; d_coeff_out is bit for bit
 * uavqp_solve_batch_device at what is handed back.  With all three attitude weights 0 that launch is skipped and every output equals that
 * of uavqp_spacetime_lbfgs_device byte for byte.
 *   attitude             validated as for uavqp_attitude_penalty_device
 *   d_attitude_peak_out  [n_traj][4] (may be NULL): d_peak of uavqp_attitude_penalty_device at what is handed back
 * WHAT THE RESULT IS: as for uavqp_spacetime_lbfgs_device, a local minimum of a piecewise smooth f with soft penalties: a limit that binds
 * may still be exceeded, d_attitude_peak_out says by how much.
 * Out of scope: as uavqp_spacetime_lbfgs_device. */
int uavqp_attitude_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                   const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                   const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                   const uavqp_attitude_params* attitude, const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out,
                                   int32_t* d_status_out, double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out,
                                   double* d_min_dist_out, int32_t* d_outside_out, double* d_attitude_peak_out);
/* The same from HOST pointers, as uavqp_spacetime_lbfgs_host. */
int uavqp_attitude_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                 double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                 const uavqp_clearance_params* clearance, const uavqp_attitude_params* attitude,
                                 const uavqp_spacetime_lbfgs_params* params, double* coeff_out, int32_t* status_out, double* objective_out,
                                 int32_t* accepted_out, double* peak_out, double* min_dist_out, int32_t* outside_out,
                                 double* attitude_peak_out);

/* Certified continuous-time bounds of solved trajectories (no reference counterpart).  Everything above that tests a limit SAMPLES the
 * trajectory; this BOUNDS it: between the knots a segment is a polynomial of degree n = 2r - 1, and the range of a polynomial over an
 * interval can be enclosed.  Per segment and quantity four numbers (outer_lo, inner_lo, inner_hi, outer_hi): the quantity stays inside
 * [outer_lo, outer_hi] for EVERY t in [0, T_i], and it takes the values inner_lo and inner_hi (up to the guard below) at some
 * t = l T_i / 2^depth.  Quantities: each axis of position, velocity, acceleration and jerk; the norms |v|, |a|, |j|; the specific thrust
 * |a + g e_z|, g = 9.81; the tilt polynomial w = z_z^2 - cos^2(tilt_max) |z|^2, z = a + g e_z (tilt <= tilt_max for all t iff w >= 0 and
 * z_z > 0 throughout).
 * Method, D = 0..3 the derivative order, m = n - D, u = t / T_i:
 *   a_k = falling(k + D, D) c[k + D] T_i^k, k = 0..m;  S = sum_k |a_k|;  Bernstein coefficients b_i = sum_{k<=i} C(i,k) / C(m,k) a_k;
 *   depth levels of midpoint de Casteljau (w_j + w_{j+1}) / 2 give 2^depth leaves (no pruning);
 *   outer = [min over all leaf coefficients - G, max + G], G = 16 (m + 1) 2^-53 S;  inner = [min, max] over the leaf END coefficients.
 *   Squared norms (degree 2m) from the undivided b: q_k = 1 / C(2m,k) sum_{i+j=k} C(m,i) C(m,j) sum_x b_{x,i} b_{x,j}, subdivided the same
 *   way, guard Gq = 32 (2m + 1) 2^-53 sum_x S_x^2; reported norms are sqrt(max(0, .)) of the guarded squares.  Thrust: q of D = 2 with g
 *   added to every z coefficient, S_z = S_z - |a_0| + |a_0 + g|.  w = [z products] - cos^2(tilt_max) q_thrust, guard Gq of the thrust,
 *   reported unrooted.  A non-finite S (Gq) makes the four numbers of the quantity NaN.
 * Outputs (each may be NULL; all NULL: UAVQP_OK, nothing done):
 *   d_range        [sum_b M_b][4][3][4]: D, axis, (outer_lo, inner_lo, inner_hi, outer_hi)
 *   d_norm         [sum_b M_b][5][4]: |v|, |a|, |j|, thrust, w, the same four numbers
 *   d_peak         [n_traj][5][4]: min (the two lower numbers) / max (the two upper) of d_norm over the segments of the trajectory
 *   d_seg_verdict  [sum_b M_b] and d_verdict [n_traj]: tests k = 0..6 = v_max, a_max, j_max, f_min, f_max, tilt_max, box.
 *                  Bit 2k (UAVQP_ENVELOPE_CERTIFIED(k)): holds for ALL t -- the outer bound, guard included, satisfies the limit.
 *                  Bit 2k + 1 (UAVQP_ENVELOPE_VIOLATED(k)): broken at a known t -- the inner bound moved TOWARDS the limit by the guard
 *                  still breaks it.  Neither: undecided at this depth.  Norms are tested on their squares against limit * limit.  A limit
 *                  of 0 switches its test off (both bits 0).  The trajectory's word is the AND of the certified bits and the OR of the
 *                  violated bits of its segments.
 *   d_box_lo / hi  [sum_b M_b][3], optional input, both or neither: one box per SEGMENT, tested on the D = 0 ranges.
 * d_status as for uavqp_limit_penalty_device: a trajectory that is not UAVQP_SOLVED, or with M < 1, gets zeros everywhere.  Non-finite
 * coefficients give non-finite bounds and no verdict bit.  Every output element is written exactly once, zeros included; min and max are
 * exact, so the bytes are the same for any grid.  One launch, asynchronous on the ctx stream, no allocation, no workspace, no read-back.
 * WHAT THE RESULT IS: a certificate, not an estimate.  After an optimiser with soft penalties this is the acceptance test: a certified
 * bit needs no sampling density to be trusted.  An undecided test is decided by a larger depth (the outer gap falls about four-fold per
 * level) or is genuinely on the limit.
 * Out of scope of THIS entry: body-rate and clearance certificates (rational / not polynomial in t) -- clearance against the distance
 * field has its own entry, uavqp_clearance_certificate_* below; pruned or adaptive subdivision; wiring the verdict into
 * uavqp_corridor_pipeline_*.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, depth outside 0..8, a limit that is negative or not finite,
 * f_max < f_min when both are set, tilt_max not 0 and outside (0, pi/2), NULL times / coeff, ragged without offsets, one box pointer
 * without the other. */
#define UAVQP_ENVELOPE_CERTIFIED(k) (1 << (2 * (k)))
#define UAVQP_ENVELOPE_VIOLATED(k) (2 << (2 * (k)))
enum { UAVQP_ENVELOPE_V_MAX = 0, UAVQP_ENVELOPE_A_MAX, UAVQP_ENVELOPE_J_MAX, UAVQP_ENVELOPE_F_MIN, UAVQP_ENVELOPE_F_MAX,
       UAVQP_ENVELOPE_TILT_MAX, UAVQP_ENVELOPE_BOX, UAVQP_ENVELOPE_TESTS };
typedef struct uavqp_envelope_params {
    int32_t struct_size;
    int32_t depth;       /* subdivision levels, 0..8 (default 4): 2^depth leaves per polynomial */
    double v_max;        /* m/s, 0: off (every limit defaults to 0) */
    double a_max;        /* m/s^2 */
    double j_max;        /* m/s^3 */
    double f_min;        /* smallest specific thrust, m/s^2 */
    double f_max;        /* largest specific thrust, m/s^2, >= f_min when both are set */
    double tilt_max;     /* rad, 0 or in (0, pi/2) */
} uavqp_envelope_params;
void uavqp_default_envelope_params(uavqp_envelope_params* out);   /* callable without a device */
int uavqp_envelope_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                          const double* d_coeff, const int32_t* d_status, const uavqp_envelope_params* params, const double* d_box_lo,
                          const double* d_box_hi, double* d_range, double* d_norm, double* d_peak, int32_t* d_seg_verdict,
                          int32_t* d_verdict);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_envelope_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                        const double* coeff, const int32_t* status, const uavqp_envelope_params* params, const double* box_lo,
                        const double* box_hi, double* range, double* norm, double* peak, int32_t* seg_verdict, int32_t* verdict);

/* Certified continuous-time clearance of solved trajectories against the distance field (no reference counterpart).  The clearance
 * penalty's min_dist, uavqp_ellipsoid_check_* and the pipeline's grid check SAMPLE: a thin pillar between two samples passes them.  This
 * BOUNDS min_t dist(p(t), O) per segment from both sides: `lower` holds for EVERY t in [0, T_i], `upper` is taken at a known t.
 * Obstacle set O: the union of the closed cubes of the occupied voxels of `esdf`, plus everything outside the map (unknown space counts
 * as occupied).  res the voxel edge, c_v = origin + (v + 0.5) res, s_v = res sqrt(sq_pos[v]) with sq_pos the exact integer squared voxel
 * distance to the nearest occupied voxel that uavqp_esdf_update_device keeps (+inf where it is INT32_MAX).  For a point p and its voxel v
 * (floor((p - origin) / res), clamped into the grid):
 *   dist(p, occupied cubes) >= s_v - (sqrt(3)/2) res - |p - c_v|       (every occupied centre is at least s_v from c_v, every point of an
 *                                                                       occupied cube within (sqrt(3)/2) res of its centre)
 *   dist(p, occupied cubes) <= s_v + |p - c_v| - res/2, 0 if sq_pos[v] = 0   (the nearest occupied cube holds the ball of radius res/2)
 * Method: the D = 0 Bernstein coefficients of uavqp_envelope_* and `depth` levels of midpoint subdivision give 2^depth leaves; the curve
 * over a leaf stays in the box of the leaf's coefficients widened per axis by the envelope's guard G_x = 16 (n + 1) 2^-53 S_x.  With m the
 * centre of that box, h its half diagonal and v the voxel of m,
 *   L_leaf = min( s_v - (sqrt(3)/2) res - |m - c_v| - h, distance from the box to the nearest face of the map ) - R
 * (the face distance is negative when the box crosses a face: a box that leaves the map cannot be certified).  Witness points are the
 * leaf end coefficients, the curve at t = l T_i / 2^depth, l = 0..2^depth:  U_l = [upper bound above] + sqrt(3) max_x G_x + R, and
 * U_l = sqrt(3) max_x G_x + R for a witness outside the map or in an occupied voxel.  R = 64 2^-53 (max_x S_x + A), A the largest
 * |coordinate| of the map plus its diagonal, is the rounding allowance of the field arithmetic.
 *   lower = max(0, min over leaves of L_leaf),  upper = min_l U_l;  the true min_t dist(p(t), O) lies in [lower, upper].
 * Outputs (each may be NULL; all NULL: UAVQP_OK, nothing done):
 *   d_clear        [sum_b M_b][2]: lower, upper
 *   d_witness      [sum_b M_b]: the l of the smallest U_l (a tie: the smallest l); the witness is at t = l T_i / 2^depth
 *   d_peak         [n_traj][2]: min of lower and min of upper over the segments of the trajectory
 *   d_seg_verdict  [sum_b M_b] and d_verdict [n_traj]: UAVQP_CLEARANCE_CERTIFIED (lower >= d_req: holds for ALL t),
 *                  UAVQP_CLEARANCE_VIOLATED (upper < d_req: broken at the witness), UAVQP_CLEARANCE_OUTSIDE (some witness point lies
 *                  outside the map); neither of the first two: undecided.  The trajectory's word is the AND of the certified bits and the
 *                  OR of the other two over its segments.
 * d_status as for uavqp_envelope_device: a trajectory that is not UAVQP_SOLVED, or with M < 1, gets zeros everywhere.  Non-finite
 * coefficients give NaN bounds, witness 0 and no bit.  Every output element is written exactly once, zeros included; min is exact and a
 * tie has a rule, so the bytes are the same for any grid.  One launch, asynchronous on the ctx stream, no allocation, no workspace, no
 * read-back; each leaf costs one gathered int32 load, each witness one more.
 * WHAT THE RESULT IS: a certificate against the VOXEL map, as conservative as the map is.  The field alone leaves an undecided band of
 * about 2 res + 2 h between lower and upper; a larger depth shrinks h, not the 2 res.
 * Out of scope: a tighter bound from a scan of the voxel's neighbourhood; adaptive subdivision; a body-rate certificate; wiring the
 * verdict into uavqp_corridor_pipeline_*.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, depth outside 0..8, d_req not finite or <= 0, esdf NULL, of
 * another device or never updated, NULL times / coeff, ragged without offsets. */
#define UAVQP_CLEARANCE_CERTIFIED 1   /* lower >= d_req: holds for ALL t */
#define UAVQP_CLEARANCE_VIOLATED 2    /* upper <  d_req: broken at the witness */
#define UAVQP_CLEARANCE_OUTSIDE 4     /* some witness point lies outside the map */
typedef struct uavqp_clearance_cert_params {
    int32_t struct_size;
    int32_t depth;       /* subdivision levels, 0..8 (default 4): 2^depth leaves per segment */
    double d_req;        /* required clearance, m, finite, > 0 (default 0.5) */
} uavqp_clearance_cert_params;
void uavqp_default_clearance_cert_params(uavqp_clearance_cert_params* out);   /* callable without a device */
int uavqp_clearance_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                       const double* d_times, const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf,
                                       const uavqp_clearance_cert_params* params, double* d_clear, int32_t* d_witness, double* d_peak,
                                       int32_t* d_seg_verdict, int32_t* d_verdict);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous); the map stays a device object. */
int uavqp_clearance_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                     const double* coeff, const int32_t* status, const uavqp_esdf* esdf,
                                     const uavqp_clearance_cert_params* params, double* clear, int32_t* witness, double* peak,
                                     int32_t* seg_verdict, int32_t* verdict);

/* Swarm separation penalty: reciprocal avoidance between the vehicles of one swarm, compared at the same instant on a clock the swarm
 * shares, with its gradients in the coefficients, the durations and the departure times (no reference counterpart: its multi_agents.launch
 * is namespacing only; the term is that of EGO-Swarm / MINCO-swarm).  It is the one penalty here that couples trajectories.
 * The batch is described as everywhere else (r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status), and in addition
 *   n_groups, d_group_offsets [n_groups + 1] int32, ascending from 0 to n_traj: swarm g is the trajectories b in [go[g], go[g+1]).
 *                 d_group_offsets NULL with n_groups == 1: the whole batch is one swarm.  The offsets are trusted on the device, as
 *                 d_seg_offsets is; the _host entry validates them.  A swarm has at most UAVQP_SWARM_MAX_VEHICLES vehicles: the _host
 *                 entry refuses a larger one, the _device entry (which cannot see the offsets) gives such a swarm Phi = NaN and zeros.
 *   d_start       [n_traj]: the departure time of each trajectory on its swarm's clock; NULL: all zero.
 * Clock samples.  t_k = clock_start + k dt (the nearest double), k = 0..N, N = n_samples; trapezoid weights om_0 = om_N = 1/2, om_k = 1
 * otherwise.  The grid does not depend on the durations: Phi is a smooth function of them, and the two vehicles of a pair are always
 * compared at the same instant.
 * Position of vehicle b at clock time t.  u = t - start_b.  u < 0: the vehicle WAITS, segment 0 at local time 0.  Otherwise segment and
 * local time come from the segment rule of uavqp_eval_batch_device at u; if the rule says past the end, or the segment is the last one
 * and the local time is at or beyond T_{M-1}, the vehicle HAS ARRIVED: last segment, local time T_{M-1} (the cap on the last segment is
 * what makes the hold continuous: the bare rule would jump by 1e-4 |v_end| there).  Held positions are evaluated from the coefficients.
 * Pair term and penalty.  delta = q_i - q_j, rho2 = (dx^2 + dy^2 + (dz / downwash)^2) / d_safe^2, x = max(0, 1 - rho2) (dimensionless,
 * smooth at delta = 0),
 *       Phi_g = dt sum_k om_k sum_{i < j in g} weight x_ijk^3
 * each unordered pair once; twice continuously differentiable.
 *   d_penalty     [n_groups] Phi_g
 *   d_grad_coeff  layout of coeff: dPhi/dc at FIXED durations.  With e_ijk = -6 weight x^2 / d_safe^2 D delta, D = diag(1, 1, 1 / downwash^2),
 *                 and G_ik = sum_{j != i} e_ijk the force on vehicle i at sample k:
 *                 grad_coeff[i][axis][m][n] = dt sum_{k in segment m} om_k G_ik[axis] t_loc^n
 *                 (a waiting sample adds to segment 0 with t_loc = 0, an arrived one to the last segment with t_loc = T_{M-1})
 *   d_grad_times  [sum_b M_b]: the EXPLICIT dPhi/dT at FIXED coefficients.  W_m = sum over the moving samples of segment m of
 *                 om_k G_ik . v_i(t_loc), P the same sum over the arrived samples with v_i = v_{M-1}(T_{M-1}):
 *                 grad_times[i][l] = -dt sum_{m > l} W_m + [l == M-1] dt P
 *                 (a moving sample's local time falls with every earlier duration; an arrived sample depends on the last duration alone)
 *   d_grad_start  [n_traj]: -dt sum_m W_m (held samples do not move with the start)
 *   d_min_sep     [n_traj]: d_safe sqrt(min rho2) over the vehicle's samples and partners; INFINITY for a vehicle without a partner
 * Each output may be NULL (all NULL: UAVQP_OK, nothing done).  As with the other penalties the TOTAL gradient in the durations is
 *       d_grad_times + uavqp_solve_backward_device(g = d_grad_coeff).grad_times
 * and the gradients in the waypoints and boundary conditions come out of that same backward call.
 * A vehicle that is not UAVQP_SOLVED (d_status NULL: all are), or has M < 1, is left out of every pair: it exerts nothing and receives
 * nothing, its own outputs are zeros and min_sep = INFINITY.  A swarm of fewer than two such vehicles has Phi = 0.  weight == 0: zeros,
 * min_sep still reported.
 * Every output element is written exactly once, zeros included: no memset is needed.  The additions are in an order fixed by indices
 * WITHIN the swarm alone: the same bytes run to run, for any grid, and for a swarm computed alone or in the middle of a batch.  No
 * floating-point atomics.  One launch, asynchronous on the ctx stream, no allocation, no read-back.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, n_samples < 1, dt or d_safe not finite or <= 0, downwash not
 * finite or < 1, weight not finite or < 0, clock_start not finite, NULL times / coeff, ragged without offsets, n_groups < 0, NULL group
 * offsets with n_groups != 1; from the _host entry also group offsets that do not ascend from 0 to n_traj or a swarm larger than
 * UAVQP_SWARM_MAX_VEHICLES.
 * The optimiser that uses the penalty (one accept / reject per SWARM): uavqp_swarm_optimize_device below.
 * Out of scope: a swarm sharded over several GPUs.  Moving or non-cooperative obstacles (trajectories that are not this batch's to move)
 * are the business of uavqp_moving_penalty_device below. */
#define UAVQP_SWARM_MAX_VEHICLES 128
typedef struct uavqp_swarm_params {
    int32_t struct_size;
    int32_t n_samples;     /* N: N + 1 clock samples (default 64) */
    double clock_start;    /* s, on the swarm's clock (default 0) */
    double dt;             /* s between clock samples (default 0.1) */
    double d_safe;         /* m: separation below which a pair is penalised (default 1.0) */
    double downwash;       /* >= 1: vertical separations count divided by this (default 1.0) */
    double weight;         /* >= 0 (default 1e3) */
} uavqp_swarm_params;
void uavqp_default_swarm_params(uavqp_swarm_params* out);   /* callable without a device */
int uavqp_swarm_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                               const double* d_coeff, const int32_t* d_status, int n_groups, const int32_t* d_group_offsets,
                               const double* d_start, const uavqp_swarm_params* params, double* d_penalty, double* d_grad_coeff,
                               double* d_grad_times, double* d_grad_start, double* d_min_sep);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_swarm_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                             const double* coeff, const int32_t* status, int n_groups, const int32_t* group_offsets, const double* start,
                             const uavqp_swarm_params* params, double* penalty, double* grad_coeff, double* grad_times, double* grad_start,
                             double* min_sep);

/* Swarm optimiser: the joint optimisation of uavqp_spacetime_optimize_device with the swarm separation penalty above in the objective and
 * ONE accept / reject per SWARM (no reference counterpart; what an EGO-Swarm / MINCO-swarm back-end gives, for a batch of swarms).  For
 * each swarm g, described by n_groups / d_group_offsets exactly as for uavqp_swarm_penalty_device, with the boundary derivatives and both
 * end waypoints of every vehicle fixed,
 *       minimise over the interior waypoints and durations of every vehicle b in g, and (start_window > 0) the departures start_b
 *           f_g = sum_{b in g} [ smooth_weight J_b + time_weight sum_i T_{b,i} + Phi_flight,b ] + Phi_swarm,g
 *       subject to   |p - p^start| <= max_move,   t_min <= T <= t_max,   |start_b - start_b^0| <= start_window
 * J_b and Phi_flight,b as in uavqp_spacetime_optimize_device, Phi_swarm,g the penalty of uavqp_swarm_penalty_device with `swarm` at the
 * departures start_b.  The swarm term couples the vehicles: a vehicle's trial means something only together with its partners' trials,
 * which is why the per-trajectory accept / reject of the single-vehicle optimisers cannot be used.
 * Gradients.  g = dPhi_flight/dc + dPhi_swarm/dc goes through ONE uavqp_solve_backward_device call per trial;
 *       df/dp_k = smooth_weight dJ/dp_k + backward(g).grad_waypoints_k
 *       df/dT_i = -smooth_weight H_i + time_weight + (explicit dPhi_flight/dT_i + explicit dPhi_swarm/dT_i) + backward(g).grad_times_i
 *       df/dstart_b = dPhi_swarm/dstart_b =: d^s_b   (already the total gradient: the coefficients do not depend on the departure)
 * Method: that of uavqp_spacetime_optimize_device -- projected gradient descent with Armijo backtracking along the projection arc, in p and
 * in u = log T -- with every quantity that is per trajectory there per SWARM here.  Directions d^p, d^u per vehicle as there; d^s_b zero
 * where the window blocks it (start_b at start_b^0 - start_window and d^s_b > 0, or at the upper end and d^s_b < 0).  One alpha and three
 * scales per swarm, fixed at the first gradient: sigma_p = initial_step_move / max |d^p|, sigma_u = initial_step_log / max |d^u|, sigma_s =
 * initial_step_start / max |d^s|, each maximum over ALL vehicles of the swarm that take part (a scale is 0 when its maximum is 0 or not
 * finite); alpha starts at 1, or at 0 if all three scales are 0.
 * Trial, every vehicle of the swarm at once: p_t = clamp(p - alpha sigma_p d^p), T_t = clamp(T exp(-alpha sigma_u d^u)), start_t =
 * clamp(start - alpha sigma_s d^s).  With need_b = sum_k (df/dp_k) . (p_k - p_t,k) + sum_i d^u_i log(T_i / T_t,i) of vehicle b,
 *       need_g = armijo_c * [ sum_b need_b + sum_b d^s_b (start_b - start_t,b) ]
 * the trial is accepted iff alpha > 0, EVERY vehicle that takes part solved at its trial point, and f_g,trial <= f_g - need_g.  Accepted:
 * every vehicle of the swarm takes its trial point, alpha *= grow; rejected: none does, alpha *= shrink.  f_g never increases.
 * Participation.  A vehicle that is not UAVQP_SOLVED at the start keeps its waypoints, durations and departure byte for byte (apart from
 * the projection of all-positive durations, as in uavqp_spacetime_optimize_device) and takes no part; the swarm penalty leaves it out of
 * every pair, and the rest of its swarm optimises without it.  A swarm with no participating vehicle, or whose f_g is not finite at the
 * start, reports (NaN, NaN) and moves nothing.
 * Host-side C++ sequencing of
 *       anchor copies, clamp, solve, flight penalty, swarm penalty, backward, step,
 *       max_iters x { solve at the trial point, flight penalty, swarm penalty at the trial departures, backward, step },
 *       solve, diagnostics
 * five launches per trial, every decision ON THE DEVICE, nothing read back, the number of launches depends on max_iters alone.  Every sum
 * is taken in an order fixed by indices inside the swarm alone: the same bytes run to run, for any grid, and for a swarm alone or in the
 * middle of a batch.  A swarm of ONE vehicle with start_window = 0 gives, byte for byte, what uavqp_spacetime_optimize_device gives for that
 * trajectory.  Asynchronous on the ctx stream (a first call of a given size allocates the workspace).
 *   d_waypoints, d_times, d_bc, d_seg_offsets, max_segments, total_segments   as for uavqp_spacetime_optimize_device (waypoints and times IN / OUT)
 *   n_groups, d_group_offsets   as for uavqp_swarm_penalty_device; trusted on the device.  A swarm of more than UAVQP_SWARM_MAX_VEHICLES takes
 *                    no part on the _device entry (objective NaN, NaN; its bytes are kept); the _host entry validates the offsets and
 *                    refuses such a swarm.
 *   d_start          [n_traj] IN: the departures, OUT: the accepted departures.  May be NULL (all zero) when start_window == 0.
 *   esdf, limits, clearance     as for uavqp_spacetime_optimize_device;  swarm: the clock, d_safe, downwash and weight, as for
 *                    uavqp_swarm_penalty_device
 *   d_coeff_out      the solve AT what is handed back: bit for bit what uavqp_solve_batch_device writes for it; d_status_out [n_traj] its
 *                    status (may be NULL)
 *   d_objective_out  [n_groups][2]: f_g at the start (after the projection of the durations), f_g at the result (NaN, NaN: took no part)
 *   d_accepted_out   [n_groups] int32 accepted trials (may be NULL)
 *   d_peak_out [n_traj][2], d_min_dist_out [n_traj], d_outside_out [n_traj] int32: the flight penalty's diagnostics at the result;
 *   d_min_sep_out [n_traj]: the swarm penalty's min_sep at the result (each may be NULL)
 *   params           uavqp_default_swarm_opt_params fills the defaults: the fields of uavqp_spacetime_params with the same names, defaults and
 *                    validity, start_window 0 (>= 0, finite), initial_step_start 0.1 s (> 0, finite).  max_iters = 0: the plain solve
 *                    after the projection of the durations, both objective columns equal.
 * UAVQP_ERR_INVALID_ARG: a wrong struct_size or an invalid field of params / swarm / limits / clearance, whatever
 * uavqp_spacetime_optimize_device refuses in the batch arguments, n_groups < 0, NULL group offsets with n_groups != 1, start_window > 0 with
 * NULL d_start; from the _host entry also group offsets that do not ascend from 0 to n_traj or a swarm larger than
 * UAVQP_SWARM_MAX_VEHICLES.
 * WHAT THE RESULT IS.  All penalties are SOFT: at finite weights two vehicles may end closer than d_safe, a limit may be exceeded by a
 * few per cent, an obstacle approached closer than the clearance asks.  The result is a LOCAL minimum of a piecewise smooth f_g: two
 * vehicles that meet head-on exactly on one line are on a saddle and do not move sideways; give them different departures or waypoints.
 * The step is the swarm's: ONE slow vehicle (a trial that does not solve, a large gradient that fixes a small scale, a rejected
 * trial) holds back the step of every vehicle of its swarm, and the scales are fixed at the FIRST gradient, as in
 * uavqp_spacetime_optimize_device; a second call re-scales.  The hard tests remain uavqp_time_reallocate_device (limits) and
 * uavqp_ellipsoid_check_* (collisions); separation is reported by d_min_sep_out on the swarm's clock samples only.
 * Between the samples it is BOUNDED by uavqp_separation_certificate_* below, the hard test of the separation.
 * Out of scope: quasi-Newton directions per swarm, capture into a graph, corridor and general-rows solves, a swarm sharded over several
 * GPUs.  Moving or non-cooperative obstacles: uavqp_moving_optimize_device below replans ONE vehicle at a time against the tracks of
 * the others, the decentralised counterpart of this entry. */
typedef struct uavqp_swarm_opt_params {
    int32_t struct_size;
    int32_t max_iters;          /* trials per swarm (default 32) */
    double smooth_weight;       /* the fields of uavqp_spacetime_params, same meaning, defaults and validity */
    double time_weight;
    double t_min;
    double t_max;
    double max_move;
    double initial_step_move;
    double initial_step_log;
    double armijo_c;
    double shrink;
    double grow;
    double start_window;        /* half width of the window around every start departure, s, >= 0, finite (default 0: departures fixed) */
    double initial_step_start;  /* largest move of a departure in the first trial, s, > 0 (default 0.1) */
} uavqp_swarm_opt_params;
void uavqp_default_swarm_opt_params(uavqp_swarm_opt_params* out);   /* callable without a device */
int uavqp_swarm_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc, int n_groups,
                                const int32_t* d_group_offsets, double* d_start, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                const uavqp_clearance_params* clearance, const uavqp_swarm_params* swarm,
                                const uavqp_swarm_opt_params* params, double* d_coeff_out, int32_t* d_status_out, double* d_objective_out,
                                int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out, int32_t* d_outside_out,
                                double* d_min_sep_out);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous; waypoints, times and start are updated in place; the map stays a
 * device object). */
int uavqp_swarm_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                              double* waypoints, double* times, const double* bc, int n_groups, const int32_t* group_offsets, double* start,
                              const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                              const uavqp_swarm_params* swarm, const uavqp_swarm_opt_params* params, double* coeff_out, int32_t* status_out,
                              double* objective_out, int32_t* accepted_out, double* peak_out, double* min_dist_out, int32_t* outside_out,
                              double* min_sep_out);

/* Certified continuous-time separation between the vehicles of a swarm (no reference counterpart): the acceptance test after
 * uavqp_swarm_optimize_*.  The swarm penalty's min_sep and the optimiser's d_min_sep_out SAMPLE the shared clock: two vehicles that cross at
 * 5 m/s each close 1 m between two samples 0.1 s apart, so a pair can pass every sample and still touch between them.  This BOUNDS, for
 * every vehicle, its separation from every partner from both sides: `lower` holds for EVERY t of the clock window [clock_start,
 * clock_start + n_cells dt] and every partner, `upper` is taken at a reported instant and partner.
 * The batch and the swarms are described exactly as for uavqp_swarm_penalty_device (r, n_traj, uniform_segments, d_seg_offsets, d_times,
 * d_coeff, d_status, n_groups, d_group_offsets, d_start), with the same UAVQP_SWARM_MAX_VEHICLES rule: the _host entry refuses a larger
 * swarm, the _device entry gives such a swarm NaN bounds, `where` {-1, 0, -1, 0} and zero words.
 * The certified curve.  The clock knots of vehicle b are the DOUBLES K_0 = start_b, K_{m+1} = fl(K_m + T_m).  For t <= K_0, q_b(t) is
 * segment 0 at local time 0 (the vehicle waits); for t in [K_m, K_{m+1}] it is segment m at local time t - K_m (real arithmetic); for
 * t >= K_M it is the last segment at T_{M-1} (it has arrived).  Pieces are closed, so at a knot both values belong to the curve (each is
 * seen by the leaf on its side of the knot; at the last instant of the window the curve is the piece the last leaf lies in).  This is the
 * swarm penalty's curve, except that it leaves out the 1e-4 s of overhang that the segment rule of uavqp_eval_batch_device allows.
 *       s_ij(t) = sqrt(dx^2 + dy^2 + (dz / downwash)^2) of q_i(t) - q_j(t)
 * Leaves.  Every clock cell is cut into 2^depth leaves: tau_w = clock_start + w (dt / 2^depth) (the nearest double), w = 0..NL,
 * NL = n_cells 2^depth; leaf l is [tau_l, tau_{l+1}].  With depth = 0 the tau_w are exactly the penalty's sample instants.
 * Method (n = 2r - 1; csrc/qp_separation_cert.h derives the constants, tests/separation_cert_reference.py restates it in numpy).  Per
 * (vehicle, leaf), every segment whose closed piece meets the leaf is restricted to it: the Bernstein coefficients of uavqp_envelope_*
 * on the segment, then two general-ratio de Casteljau splits at lambda_1 = lb / T_m (left half kept) and lambda_2 = la / lb (right half
 * kept), la = max(tau_l - K_m, 0), lb = min(tau_{l+1} - K_m, T_m), both ratios clamped to [0, 1]; a hold is a constant polynomial.  A
 * leaf inside ONE piece (all waiting, all arrived, or K_m <= tau_l and tau_{l+1} <= K_{m+1} on the doubles) gives a SINGLE entry, the
 * 3 x (n + 1) coefficients; a leaf that straddles a knot, the departure or the arrival gives a BOX entry, the per-axis [lo, hi] over the
 * coefficients of all its pieces.  Guard per axis G_x = (64 (n + 1) + 2 n kappa) 2^-53 S_x, S_x = sum_k |c_k T^k| of the segment, kappa =
 * max(|K_m|, |K_{m+1}|) / T_m (K_{m+1} is a rounded sum), the largest over the pieces of the entry.
 * Pair (i, j) on a leaf: both single, the range of q_i - q_j per axis is [min_k, max_k] of b_ik - b_jk (both are Bernstein in the same
 * parameter over the same leaf, so correlated motion cancels); otherwise the interval difference of the two boxes (the box of a single
 * entry: min / max of its coefficients).  Widened by G_i + G_j; g_x = max(0, lo_x, -hi_x);
 *       L = sqrt(g_x^2 + g_y^2 + (g_z / downwash)^2) - R,                          R = 16 2^-53 (sum_x max(|lo_x|, |hi_x|))
 *       U = s_ij(tau_w) + sqrt(3) max_x (G_ix + G_jx) + R_w  at the leaf ends,      R_w = 16 2^-53 (|d_x| + |d_y| + |d_z|) of the difference
 *   lower_i = max(0, min over j and leaves of L),  upper_i = min over j and witnesses of U;  min_t min_j s_ij(t) over the window lies in
 * [lower_i, upper_i].  A tie goes to the smaller partner, then the smaller index.
 * Outputs (each may be NULL; all NULL: UAVQP_OK, nothing done; every element is written exactly once):
 *   d_lower          [n_traj]: holds for every t of the window and every partner
 *   d_upper          [n_traj]: taken at a witness
 *   d_where          [n_traj][4] int32: {partner of lower, leaf of lower, partner of upper, witness index w of upper (the instant tau_w)};
 *                    partners are batch indices, -1 (and index 0) when there is none
 *   d_verdict        [n_traj] int32: UAVQP_SEPARATION_CERTIFIED (lower >= d_req: holds for ALL t of the window), UAVQP_SEPARATION_VIOLATED
 *                    (upper < d_req: broken at the witness), neither: undecided at this depth; UAVQP_SEPARATION_MOVING: the vehicle is
 *                    still under way at the end of the window (K_M > tau_NL) -- the certificate says nothing about what happens afterwards
 *   d_group_verdict  [n_groups] int32: AND of the certified bit, OR of the other bits over the vehicles of the swarm that take part; 0 for
 *                    a swarm in which none does
 * A vehicle that is not UAVQP_SOLVED (d_status NULL: all are), or has M < 1, is left out of every pair; its outputs are INFINITY, INFINITY,
 * {-1, 0, -1, 0}, 0.  A solved vehicle without a partner gets INFINITY bounds and counts as certified.  Non-finite coefficients or a
 * duration <= 0 in a piece the window meets give the vehicle AND its partners NaN bounds, {-1, 0, -1, 0} and no bits.
 * Every min is exact and a pair's numbers are the same bits from both sides: the same bytes for any grid, run to run, and for a swarm
 * computed alone or in the middle of a batch.  One launch, asynchronous on the ctx stream, no allocation, no workspace, no atomics, no
 * read-back.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size, depth outside 0..6, n_cells < 1 or above
 * UAVQP_SEPARATION_MAX_CELLS, dt or d_req not finite or <= 0, downwash not finite or < 1, clock_start not finite, NULL times / coeff, ragged
 * without offsets, n_groups < 0, NULL group offsets with n_groups != 1; from the _host entry also group offsets that do not ascend from 0
 * to n_traj or a swarm larger than UAVQP_SWARM_MAX_VEHICLES.
 * Out of scope: splitting a straddling leaf at the pair's merged knots (without it a straddling leaf falls back to boxes); a degree-2n
 * squared-distance polynomial per pair; adaptive subdivision; non-cooperative obstacles; wiring the verdict into uavqp_swarm_optimize_*.
 * Against obstacle tracks (uavqp_moving_penalty_device below) use uavqp_moving_certificate_device: unlike this entry run on a vehicle and
 * its tracks as ONE group, it takes radii into account, has no cap on a set, spends nothing on obstacle-obstacle pairs and certifies the
 * trajectory's own flight instead of a clock window. */
#define UAVQP_SEPARATION_CERTIFIED 1   /* lower >= d_req: holds for ALL t of the window */
#define UAVQP_SEPARATION_VIOLATED 2    /* upper <  d_req: broken at the witness */
#define UAVQP_SEPARATION_MOVING 4      /* still under way at the end of the window */
#define UAVQP_SEPARATION_MAX_CELLS 1048576
typedef struct uavqp_separation_params {
    int32_t struct_size;
    int32_t depth;        /* 0..6: every clock cell is cut into 2^depth leaves (default 2) */
    int32_t n_cells;      /* N >= 1 cells of dt: the window is [clock_start, clock_start + N dt] (default 64) */
    double clock_start;   /* as in uavqp_swarm_params (default 0) */
    double dt;            /* (default 0.1) */
    double downwash;      /* (default 1.0) */
    double d_req;         /* required separation, m, finite, > 0 (default 1.0) */
} uavqp_separation_params;
void uavqp_default_separation_params(uavqp_separation_params* out);   /* callable without a device */
int uavqp_separation_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                        const double* d_times, const double* d_coeff, const int32_t* d_status, int n_groups,
                                        const int32_t* d_group_offsets, const double* d_start, const uavqp_separation_params* params,
                                        double* d_lower, double* d_upper, int32_t* d_where, int32_t* d_verdict, int32_t* d_group_verdict);
/* The same from HOST pointers (H2D copy, run, D2H copy, synchronous). */
int uavqp_separation_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                      const double* coeff, const int32_t* status, int n_groups, const int32_t* group_offsets,
                                      const double* start, const uavqp_separation_params* params, double* lower, double* upper,
                                      int32_t* where, int32_t* verdict, int32_t* group_verdict);

/* Moving-obstacle penalty: a trajectory against obstacles that MOVE and are not this batch's to move -- the committed trajectories the
 * other vehicles of a decentralised fleet have broadcast, a predicted pedestrian, another aircraft (no reference counterpart; the term is
 * that of EGO-Swarm, where each vehicle replans on its own against the trajectories of the others).  The shape of
 * uavqp_attitude_penalty_device, with its gradients in the coefficients, the durations and the departure.
 * Obstacle tracks.  An obstacle is a trajectory in the library's own format: the SAME r as the batch, coefficients in the layout of coeff,
 * durations, and a start on the clock.  A committed trajectory is handed over as it is; a constant-velocity or constant-acceleration
 * prediction is a one-segment track whose higher coefficients are zero.  uavqp_moving_obstacles describes them; its pointers are device
 * pointers for the _device entries and host pointers for the _host entries:
 *   n_obs, uniform_segments, seg_offsets, times, coeff   the obstacle batch, described as a trajectory batch is everywhere else
 *   start  [n_obs] the departure of each obstacle on the clock (NULL: zeros);  radius [n_obs] finite, >= 0 (NULL: zeros)
 *   n_sets, set_offsets [n_sets + 1] int32 ascending from 0 to n_obs: set k is the obstacles [so[k], so[k+1]); no cap on a set's size, an
 *          empty set is allowed.  set_offsets NULL with n_sets == 1: the whole obstacle batch is set 0.
 *   traj_set [n_traj] int32: the set trajectory b avoids, -1 for none; NULL with n_sets == 1: every trajectory avoids set 0
 *   traj_start [n_traj]: the departure of each trajectory of the batch on the same clock (NULL: zeros)
 * Offsets and traj_set are trusted on the device, as d_seg_offsets is; the _host entries validate that the set offsets ascend from 0 to
 * n_obs, that traj_set lies in [-1, n_sets), the radii, and the CSR offsets of the obstacle batch.
 * Samples.  For trajectory b with departure S = traj_start[b]: the clock knots are the DOUBLES K_0 = S, K_{m+1} = fl(K_m + T_m) (the
 * convention of uavqp_separation_certificate_device); sample s = 0..K of segment m is at local time t = tau_s T_m, tau_s = s / K,
 * K = samples_per_seg, at clock time t_abs = fma(tau_s, T_m, K_m); the trapezoid weights om_s are those of uavqp_limit_penalty_device.
 * Obstacle o at t_abs: exactly the position rule of uavqp_swarm_penalty_device at u = t_abs - start_o (u < 0: it waits, segment 0 at local
 * time 0; otherwise the segment rule of uavqp_eval_batch_device; arrived: last segment at T_{M-1}, with the cap on the last segment).  Its
 * velocity o'(t_abs) is that of the located segment, and zero while the obstacle is held (waiting or arrived).
 * Term.  delta = q(t) - o(t_abs), D_o = d_safe + radius_o, rho2 = (dx^2 + dy^2 + (dz / downwash)^2) / D_o^2, x_o = max(0, 1 - rho2):
 *       phi = weight sum_{o in set} x_o^3                     Phi = sum_m (T_m / K) sum_s om_s phi
 *       e_o = -6 weight x_o^2 / D_o^2 diag(1, 1, 1 / downwash^2) delta
 *       G   = sum_o e_o                    (dphi/dq)
 *       Gt  = -sum_o e_o . o'(t_abs)       (dphi/dt_abs)
 *       Q_m = sum_s om_s Gt
 *   d_penalty     [n_traj] Phi
 *   d_grad_coeff  layout of coeff: grad_coeff[axis][m][n] = (T_m / K) sum_s om_s G[axis] t^n, at FIXED durations
 *   d_grad_times  [sum_b M_b]: the EXPLICIT dPhi/dT_l at FIXED coefficients
 *                 = Phi_l / T_l + (T_l / K) sum_s om_s tau_s (G . v(t) + Gt) + sum_{m > l} (T_m / K) Q_m
 *                 (the last term is what no other penalty has: a later segment's samples move on the clock with every earlier duration)
 *   d_grad_start  [n_traj]: dPhi/dS = sum_m (T_m / K) Q_m -- already the total gradient, the coefficients do not depend on the departure
 *   d_min_gap     [n_traj]: the smallest sqrt(dx^2 + dy^2 + (dz / downwash)^2) - radius_o over the samples and the obstacles of the set;
 *                 INFINITY for a trajectory without an obstacle
 *   d_nearest     [n_traj] int32: the index in the obstacle batch of the obstacle that attains d_min_gap, -1 when there is none; a tie
 *                 goes to the smaller index
 * Each output may be NULL (all NULL: UAVQP_OK, nothing done).  As with every other penalty the TOTAL gradients in durations, waypoints and
 * boundary derivatives are d_grad_times + uavqp_solve_backward_device(g = d_grad_coeff).
 * A trajectory that is not UAVQP_SOLVED (d_status NULL: all are), has M < 1, has set -1 or an empty set gets zeros, INFINITY and -1.
 * weight == 0: zeros, d_min_gap and d_nearest still reported.  Every output element is written exactly once, zeros included.  No
 * floating-point atomics; the order of every addition is fixed by sample, obstacle and segment indices alone (the sum over later segments
 * runs from the LAST segment down): the same bytes run to run, for any grid, and for a trajectory alone or in the middle of a batch.
 * One launch, asynchronous on the ctx stream, no allocation, no workspace, no read-back.
 * WHAT THE RESULT IS: a SOFT penalty on SAMPLES.  d_min_gap is the check afterwards, on the samples only; between them nothing is bounded
 * (the bound for every t: uavqp_moving_certificate_device below).  The obstacle's position is not smooth in
 * t_abs where it departs or arrives with a non-zero velocity; the gradient is that of the piece the sample lies in.
 * UAVQP_ERR_INVALID_ARG: r not 3 / 4, a negative count, a wrong struct_size of either struct, samples_per_seg < 1, d_safe not finite or
 * <= 0, downwash not finite or < 1, weight not finite or < 0, NULL times / coeff, ragged without offsets, NULL obstacles, n_obs < 0, a
 * negative uniform_segments of the obstacles, NULL obstacle times / coeff with n_obs > 0, ragged obstacles without offsets, n_sets < 0,
 * NULL set_offsets or NULL traj_set with n_sets != 1; from the _host entry also set offsets that do not ascend from 0 to n_obs, a traj_set
 * outside [-1, n_sets), a radius that is negative or not finite, obstacle offsets that do not ascend from 0.
 * Out of scope: departures as optimisation variables, obstacles that appear or vanish inside a window, a per-obstacle cull, wiring into
 * uavqp_swarm_optimize_* or the corridor pipeline. */
typedef struct uavqp_moving_params {
    int32_t struct_size;
    int32_t samples_per_seg;   /* K: K + 1 sample points per segment (default 8) */
    double d_safe;             /* m: gap to an obstacle's surface below which it is penalised, finite, > 0 (default 1.0) */
    double downwash;           /* >= 1: vertical separations count divided by this (default 1.0) */
    double weight;             /* >= 0 (default 1e3) */
} uavqp_moving_params;
typedef struct uavqp_moving_obstacles {
    int32_t struct_size;
    int32_t n_obs;
    int32_t uniform_segments;      /* of the obstacle batch; 0: ragged, seg_offsets [n_obs + 1] */
    int32_t n_sets;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const double* start;           /* [n_obs] or NULL: zeros */
    const double* radius;          /* [n_obs] or NULL: zeros */
    const int32_t* set_offsets;    /* [n_sets + 1], or NULL with n_sets == 1 */
    const int32_t* traj_set;       /* [n_traj], or NULL with n_sets == 1 */
    const double* traj_start;      /* [n_traj] or NULL: zeros */
} uavqp_moving_obstacles;
void uavqp_default_moving_params(uavqp_moving_params* out);   /* callable without a device */
int uavqp_moving_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                                const double* d_coeff, const int32_t* d_status, const uavqp_moving_obstacles* obstacles,
                                const uavqp_moving_params* params, double* d_penalty, double* d_grad_coeff, double* d_grad_times,
                                double* d_grad_start, double* d_min_gap, int32_t* d_nearest);
/* The same from HOST pointers, those inside `obstacles` included (H2D copy, run, D2H copy, synchronous). */
int uavqp_moving_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                              const double* coeff, const int32_t* status, const uavqp_moving_obstacles* obstacles,
                              const uavqp_moving_params* params, double* penalty, double* grad_coeff, double* grad_times, double* grad_start,
                              double* min_gap, int32_t* nearest);

/* uavqp_attitude_optimize_device with the moving-obstacle penalty inside the objective: per trajectory
 *       minimise  f(p, T) = [the objective of uavqp_attitude_optimize_device] + Phi_moving(c*(p, T), T)
 * Phi_moving exactly the formula of uavqp_moving_penalty_device with `obstacles` and `moving`.  Variables, bounds, directions, the ONE
 * accept / reject per trajectory and trial, the arguments, the outputs and the parameters are those of uavqp_attitude_optimize_device;
 * `attitude` may be NULL here: no attitude term (d_attitude_peak_out is then not written).  Departures (traj_start) are FIXED.
 * Sequencing: one more accumulating launch per trial, behind the attitude launch and before the ONE backward pass -- at most six
 * launches per trial, none that depends on the data, nothing read back.  d_objective_out holds f INCLUDING Phi_moving.  With
 * moving->weight == 0, or no trajectory that can have an obstacle (n_obs == 0 or n_sets == 0), that launch is skipped and every shared
 * output equals uavqp_attitude_optimize_device byte for byte -- with attitude NULL as well, uavqp_spacetime_lbfgs_device.
 *   d_min_gap_out [n_traj], d_nearest_out [n_traj] int32 (each may be NULL): d_min_gap / d_nearest of uavqp_moving_penalty_device at what
 *                 is handed back
 * WHAT THE RESULT IS: as for uavqp_spacetime_lbfgs_device, a local minimum of a piecewise smooth f with soft penalties; d_min_gap_out says
 * how close the result still comes, on the samples.
 * UAVQP_ERR_INVALID_ARG: what uavqp_attitude_optimize_device refuses (a NULL attitude excepted) and what uavqp_moving_penalty_device
 * refuses in `obstacles` and `moving`.
 * Out of scope: as uavqp_moving_penalty_device and uavqp_spacetime_lbfgs_device. */
int uavqp_moving_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                 const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                 const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                 const uavqp_attitude_params* attitude, const uavqp_moving_obstacles* obstacles,
                                 const uavqp_moving_params* moving, const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out,
                                 int32_t* d_status_out, double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out,
                                 double* d_min_dist_out, int32_t* d_outside_out, double* d_attitude_peak_out, double* d_min_gap_out,
                                 int32_t* d_nearest_out);
/* The same from HOST pointers, those inside `obstacles` included, as uavqp_attitude_optimize_host. */
int uavqp_moving_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                               double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                               const uavqp_clearance_params* clearance, const uavqp_attitude_params* attitude,
                               const uavqp_moving_obstacles* obstacles, const uavqp_moving_params* moving,
                               const uavqp_spacetime_lbfgs_params* params, double* coeff_out, int32_t* status_out, double* objective_out,
                               int32_t* accepted_out, double* peak_out, double* min_dist_out, int32_t* outside_out, double* attitude_peak_out,
                               double* min_gap_out, int32_t* nearest_out);

/* Certified continuous-time gap between solved trajectories and moving-obstacle tracks (no reference counterpart): the acceptance test
 * after uavqp_moving_optimize_*.  d_min_gap of the penalty and d_min_gap_out of the optimiser SAMPLE: a vehicle and a track that close at
 * 10 m/s move 1.25 m against each other between two of the default eight samples of a 1 s segment, so the samples can report a gap of
 * 0.65 m where the true one is 0.2 m.  This BOUNDS, for every segment of every trajectory and every obstacle of its set, the minimum over
 * the segment's flight time of
 *       gap_o(t) = sqrt(dx^2 + dy^2 + (dz / downwash)^2) - radius_o     of q(t) - o(t_abs)
 * from both sides: `lower` holds for EVERY t of the segment, `upper` is taken at a reported instant and obstacle.
 * The batch is described as everywhere else; `obstacles` is taken exactly as uavqp_moving_penalty_* takes it (the same fields, the same
 * NULL conventions, traj_start the departures of the batch; device pointers for _device, host pointers for _host).
 * The certified curves.  Trajectory b departs at S = traj_start[b]; its clock knots are the DOUBLES K_0 = S, K_{m+1} = fl(K_m + T_m) (as in
 * the penalty and in uavqp_separation_certificate_device); at local time s of segment m it is at q_m(s) and the clock shows K_m + s.
 * Obstacle o is the curve of uavqp_separation_certificate_device on that clock, with its knots K^o_0 = start_o, K^o_{m+1} = fl(K^o_m +
 * T^o_m): it waits at segment 0, local time 0, before start_o; follows CLOSED pieces (at a knot both values belong to the curve); stays at
 * the end of its last segment after arrival.  It does NOT have the 1e-4 s of overhang of the penalty's sampling rule.
 * Leaves.  Leaf l = 0..2^depth - 1 of segment m is the local time [l, l + 1] T_m / 2^depth; its clock ends are ta = fma(l 2^-depth, T_m,
 * K_m) and tb = fma((l + 1) 2^-depth, T_m, K_m), one rounding each.  Witness l = 0..2^depth is the local time l T_m / 2^depth; with the
 * default depth 3 the witnesses are the samples of the default uavqp_moving_params.
 * Method (n = 2r - 1; csrc/qp_moving_cert.h derives the constants, tests/moving_cert_reference.py restates it in numpy).  The trajectory
 * over a leaf: the Bernstein coefficients of uavqp_envelope_* and depth midpoint subdivisions, guard G_x = 16 (n + 1) 2^-53 S_x (the leaf
 * of uavqp_clearance_certificate_*).  The obstacle over [ta, tb]: the entry of uavqp_separation_certificate_device -- SINGLE (its
 * 3 x (n + 1) coefficients, Bernstein in the same parameter as the leaf's, so correlated motion cancels) when the leaf lies in one piece,
 * otherwise BOX (per-axis [lo, hi] over the pieces the leaf meets) -- with the guard G^o_x = (64 (n + 1) + 4 n kappa_o) 2^-53 S_x, kappa_o =
 * max(|K^o_m|, |K^o_{m+1}|, |ta|, |tb|) / T^o_m (the rounded ta, tb shift the restriction by at most 2^-53 max(|ta|, |tb|)); a held obstacle
 * has the separation certificate's rule.  Pair (leaf, o), Gs_x = G_x + G^o_x: the range of q - o per axis is [min_k, max_k] of w_k - b^o_k
 * (single) or the interval difference with the box of the leaf's coefficients (box), widened by Gs_x; g_x = max(0, lo_x, -hi_x);
 *       L = max(0, sqrt(g_x^2 + g_y^2 + (g_z / downwash)^2) - R) - radius_o,        R = 16 2^-53 sum_x max(|lo_x|, |hi_x|)
 *       U = |d|_downwash + sqrt(3) max_x Gs_x + 16 2^-53 (|d_x| + |d_y| + |d_z|) - radius_o,   d the difference at a witness
 *   lower = min over obstacles and leaves of L (negative: the vehicle is inside a radius), upper = min over obstacles and witnesses of U;
 *   min_t min_o gap_o(t) over the segment lies in [lower, upper].  A tie goes to the smaller obstacle, then the smaller leaf / witness.
 * A rounded ta (tb) is not trusted to lie on the right side of an obstacle knot (a track may JUMP at a knot): an end that is not exactly
 * l 2^-depth T_m + K_m stands for [t - 2^-52 |t|, t + 2^-52 |t|], which holds the real end; the pieces a leaf meets, and whether it lies in
 * ONE, are decided on that widened leaf (a piece met through the margin alone comes in as its end point and makes the entry a BOX), and
 * where an obstacle knot lies in the interval of an end of a leaf that is not in one piece, that obstacle gives no witness at that end.
 * Exact ends (dyadic durations and departures) stand for themselves: a track that flies the trajectory's own dyadic knots is SINGLE on
 * every leaf; with knots that are no dyadic numbers it is a BOX on the leaves that end at a knot.  Where a leaf end and an obstacle knot
 * coincide exactly, each of the two values at the knot is seen by the leaf on its side (the rule of the separation certificate).
 * Outputs (each may be NULL; all NULL: UAVQP_OK, nothing done; every element is written exactly once):
 *   d_gap          [sum_b M_b][2]: lower, upper of the segment
 *   d_where        [sum_b M_b][4] int32: {obstacle of lower, leaf of lower, obstacle of upper, witness index l of upper (local time
 *                  l T_m / 2^depth)}; obstacles are indices into the obstacle batch; {-1, 0, -1, 0} when there is none
 *   d_peak         [n_traj][2]: min of lower, min of upper over the segments
 *   d_seg_verdict  [sum_b M_b] int32: UAVQP_MOVING_CERT_CERTIFIED (lower >= d_req: holds for ALL t of the segment),
 *                  UAVQP_MOVING_CERT_VIOLATED (upper < d_req: broken at the witness), neither: undecided at this depth
 *   d_verdict      [n_traj] int32: AND of the certified bits, OR of the violated bits of the segments
 * A solved trajectory whose set is -1 or empty: INFINITY bounds, {-1, 0, -1, 0}, certified (the rule of the separation certificate for a
 * vehicle without a partner; its coefficients are not looked at).  A trajectory that is not UAVQP_SOLVED (d_status NULL: all are) or has
 * M < 1: INFINITY, INFINITY, {-1, 0, -1, 0}, word 0.  Non-finite coefficients or a duration <= 0 in the segment, or in an obstacle piece one
 * of its leaves meets: NaN bounds, {-1, 0, -1, 0} and no bit for that segment; the trajectory's peak is NaN and its word 0.  A NaN duration
 * loses the knot clock as well: every LATER segment of that trajectory gets the same (a duration <= 0 spoils its own segment alone).
 * Every min is exact: the same bytes for any grid, run to run, and for a trajectory alone or in the middle of a batch.  One launch,
 * asynchronous on the ctx stream, no allocation, no workspace, no atomics, no read-back.
 * UAVQP_ERR_INVALID_ARG: what uavqp_moving_penalty_* refuses in the batch and in `obstacles`, with the same precedence; a wrong
 * struct_size, depth outside 0..6, downwash not finite or < 1, d_req not finite or <= 0.
 * Out of scope: adaptive subdivision; splitting a leaf at an obstacle's knots (a straddling leaf falls back to a box); a per-obstacle
 * cull; the time before departure and after arrival; wiring the verdict into uavqp_moving_optimize_*. */
#define UAVQP_MOVING_CERT_CERTIFIED 1   /* lower >= d_req: holds for ALL t of the segment */
#define UAVQP_MOVING_CERT_VIOLATED 2    /* upper <  d_req: broken at the witness */
typedef struct uavqp_moving_cert_params {
    int32_t struct_size;
    int32_t depth;      /* 0..6: 2^depth leaves per segment (default 3: the witnesses are then the default samples of the penalty) */
    double downwash;    /* finite, >= 1 (default 1.0) */
    double d_req;       /* required gap to an obstacle's surface, m, finite, > 0 (default 1.0) */
} uavqp_moving_cert_params;
void uavqp_default_moving_cert_params(uavqp_moving_cert_params* out);   /* callable without a device */
int uavqp_moving_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                    const double* d_times, const double* d_coeff, const int32_t* d_status,
                                    const uavqp_moving_obstacles* obstacles, const uavqp_moving_cert_params* params, double* d_gap,
                                    int32_t* d_where, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict);
/* The same from HOST pointers, those inside `obstacles` included (H2D copy, run, D2H copy, synchronous). */
int uavqp_moving_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                  const double* coeff, const int32_t* status, const uavqp_moving_obstacles* obstacles,
                                  const uavqp_moving_cert_params* params, double* gap, int32_t* where, double* peak, int32_t* seg_verdict,
                                  int32_t* verdict);

/* Batched evaluation of solved trajectories on a uniform time grid.
 * Replaces, for a whole batch, PolyTraj::evaluatePos / evaluateVel / evaluateAcc
 * (src/planner/traj_utils/include/traj_utils/poly_traj.hpp:74-168) as driven by poly_traj_server's
 * 100 Hz timer (traj_server/src/poly_traj_server.cpp:33-37) and PolyTraj::getTraj (poly_traj.hpp:175-187),
 * and the caller-side sampling loop of test_minimum_jerk.cpp:79-92.
 *   t_s = t0 + s*dt, s = 0..n_samples-1, is trajectory-global time; the segment is found with the
 *   reference's rule (walk while t > T_idx + 1e-4, subtracting; past the end clamp to the last segment's
 *   end, poly_traj.hpp:77-88).
 *   what: bit 0 position, bit 1 velocity, bit 2 acceleration; K = popcount(what) outputs per sample.
 *   d_out [n_traj][n_samples][K][3] float64 (pos, vel, acc order; xyz interleaved = Eigen::Vector3d).
 * The segment rule in full (shared by the four samplers below; float64, the same subtractions in the same order): idx = 0; while idx < M and
 * t > T_idx + 1e-4 (the sum rounded once, the comparison strict): t -= T_idx, ++idx; if idx == M: idx = M - 1, t = T_{M-1}.  So a sample exactly on
 * a knot, or beyond it by no more than the slack, belongs to the EARLIER segment, whose polynomial is then evaluated past its end; t < 0 is
 * segment 0 extrapolated backwards; every sample past the end is the end point of the last segment (velocity and acceleration there too).
 * Only the low three bits of `what` count ((what & 7) == 0: UAVQP_ERR_INVALID_ARG).  A zero-segment trajectory gets rows of zeros.  n_samples == 0
 * or n_traj == 0 writes nothing.  d_out needs no more than the 8-byte alignment of a double.
 * d_coeff / d_times / d_seg_offsets: the arrays of uavqp_solve_batch_device.  Asynchronous on the ctx stream. */
int uavqp_eval_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                            const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                            int what, double* d_out);

/* Batched PolyTraj::getTraj + getLength + getMeanVel (src/planner/traj_utils/include/traj_utils/poly_traj.hpp:175-207), the two
 * evaluator members without a per-sample output: positions sampled at t = 0, dt, 2 dt, ... while t < total time (the reference's
 * dt is the constant 0.01 and its t is ACCUMULATED in floating point: the sample count follows that accumulation exactly, so a
 * total time that is a multiple of dt -- the reference's own 1.0 s per segment -- gives the reference's count), length = sum of the
 * chord lengths between consecutive samples, mean velocity = length / total time.
 * The positions themselves are evaluated at t_s = s * dt (the float64 product, not the accumulated t: the two differ by rounding only)
 * through the segment rule of uavqp_eval_batch_device.  total time = the durations added in order.  One sample (dt >= total time): length 0.
 * A zero-segment trajectory has total time 0: no sample, length 0, and mean velocity 0 / 0 = NaN -- the reference's length / total, unguarded.
 * dt must be positive and finite (else UAVQP_ERR_INVALID_ARG).
 *   d_length / d_mean_vel [n_traj] float64, d_n_samples [n_traj] int32: any of them may be NULL.  Asynchronous on the ctx stream. */
int uavqp_traj_length_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                             const double* d_times, const double* d_coeff, double dt, double* d_length, double* d_mean_vel,
                             int32_t* d_n_samples);

/* Batched SE(3) ellipsoid collision check of solved trajectories against an obstacle point cloud
 * (SURVEY.md section 8-f, N4).  Replaces, for every sample of every trajectory, KinoAstar::isCollisionFree(pt, acc)
 * (src/planner/path_searching/src/kino_astar.cpp:721-758): body axis b3 = normalize(acc + 9.81 z),
 * b2 = normalize(b3 x (1,0,0)), b1 = normalize(b2 x b3), E = Rot diag(robot_r, robot_r, robot_h) Rot', and a
 * sample collides when some obstacle point o within robot_r + 0.1 of it has |E^-1 (o - p)| <= 1.  The kd-tree
 * radius search of the reference is an exhaustive scan here.  Candidate set: |o - p|^2 <= (robot_r + 0.1)^2 in float64; the
 * reference's PCL search works on float32 points with a float radius (kino_astar.cpp:747-748), so a point within float rounding
 * of the search sphere may be a candidate in one and not in the other.  The VERDICT is unaffected: the ellipsoid (semi-axes
 * robot_r, robot_r, robot_h <= robot_r) lies strictly inside that sphere, so such a point never passes |E^-1 (o - p)| <= 1.
 *   samples: t_s = t0 + s*dt, position and acceleration from the polynomials (segment rule of uavqp_eval_batch_device)
 *   d_obstacles [n_obs][3] float64
 *   d_first_hit [n_traj] int32: index of the first colliding sample, n_samples if the trajectory is collision-free
 *   d_flags     [n_traj][n_samples] uint8 (1 = collides), may be NULL (d_first_hit is the same with and without it)
 * Degenerate attitudes: acc = (0, 0, -9.81) (no thrust: b3 is the zero vector) and acc = (a, 0, -9.81) (b3 parallel to x: b3 x (1,0,0) is the
 * zero vector) leave axes that cannot be normalised.  The reference's E is then singular, E^-1 (o - p) is not a number and its test
 * |E^-1 (o - p)| <= 1 is false for every point (the same in oracle/ellipsoid.c, whose division by the zero norm gives NaN axes): such a sample
 * is reported COLLISION-FREE whatever the cloud holds, by both entry points.  A zero-segment trajectory has nothing to sample: flags 0,
 * first_hit = n_samples. */
int uavqp_ellipsoid_check_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                 const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                 const double* d_obstacles, int n_obs, double robot_r, double robot_h,
                                 int32_t* d_first_hit, uint8_t* d_flags);

/* Uniform grid over an obstacle point cloud and the ellipsoid check that queries it instead of scanning every point:
 * the batched stand-in for the kd-tree radius search of KinoAstar::isCollisionFree
 * (src/planner/path_searching/src/kino_astar.cpp:747-750, kdtree radiusSearch(pt, robot_r + 0.1)).
 *   uavqp_obstacle_grid_build_device: buckets d_obstacles [n_obs][3] by cell (cell_size > 0; robot_r + 0.1 makes a
 *     query visit 27 cells; clouds too large for 2^22 cells get larger cells).  Synchronous (sizes depend on the
 *     cloud's bounds); the grid owns a sorted copy of the points, d_obstacles may be freed afterwards.
 *   uavqp_ellipsoid_check_grid_device: arguments and results of uavqp_ellipsoid_check_device with the grid in place
 *     of the raw cloud -- the same candidate set as uavqp_ellipsoid_check_device and the same arithmetic per candidate, hence
 *     flags identical to it.
 * No reference counterpart as a batch; the per-query semantics are the reference's. */
typedef struct uavqp_grid uavqp_grid;
int uavqp_obstacle_grid_build_device(uavqp_ctx* ctx, const double* d_obstacles, int n_obs, double cell_size, uavqp_grid** out_grid);
int uavqp_obstacle_grid_destroy(uavqp_ctx* ctx, uavqp_grid* grid);
int uavqp_ellipsoid_check_grid_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                      const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                      const uavqp_grid* grid, double robot_r, double robot_h, int32_t* d_first_hit,
                                      uint8_t* d_flags);

/* Corridor boxes from an obstacle point cloud (SURVEY.md section 8-d config 5 "ellipsoid-derived corridor widths",
 * 8-f N4).  No reference counterpart as a function: it turns the reference's SE(3) collision test
 * KinoAstar::isCollisionFree(pt, acc) (src/planner/path_searching/src/kino_astar.cpp:721-758) into the box
 * lo <= p <= hi that uavqp_solve_corridor_batch_device puts in place of the waypoint rows
 * (minimum_control.cpp:34-42,118-124).  For every waypoint row w (n_rows = sum over trajectories of M_b + 1):
 *   attitude: b3 = normalize(acc + 9.81 z), b2 = normalize(b3 x (1,0,0)), b1 = normalize(b2 x b3)
 *             (kino_astar.cpp:724-727), E = Rot diag(robot_r, robot_r, robot_h) Rot' (:729-737), with acc the
 *             acceleration of the solved polynomials d_coeff at that knot, or 0 (hover) when d_coeff is NULL;
 *   clearance g = min over ALL obstacle points o of |E^-1 (o - w)|   (the reference's collision metric, :751-753;
 *             +inf for an empty cloud; g <= 1 means the waypoint itself collides);
 *   half-widths h_i = min(h_max, max(0, g - 1) / (3 |E^-1 e_i|)), i = x, y, z;  lo = w - h, hi = w + h.
 * Guarantee: for any offset d with |d_i| <= h_i and any obstacle o, |E^-1 (o - w - d)| >= g - sum_i |d_i| |E^-1 e_i|
 * >= 1, i.e. the robot ellipsoid (same attitude) translated anywhere in the box contains no obstacle point.
 * A colliding waypoint gets h = 0: lo == hi, the reference's equality row.  First/last rows of a trajectory get
 * lo == hi == w (the corridor solver fixes the end points).
 *   d_times      may be NULL when d_coeff is NULL
 *   d_obstacles  [n_obs][3] float64 (exhaustive scan, like uavqp_ellipsoid_check_device)
 *   d_corr_lo / d_corr_hi  [n_rows][3] float64 out
 *   d_clearance  [n_rows] float64 out (g), may be NULL
 * Asynchronous on the ctx stream. */
int uavqp_corridor_from_cloud_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                     int n_rows, const double* d_waypoints, const double* d_times, const double* d_coeff,
                                     const double* d_obstacles, int n_obs, double robot_r, double robot_h, double h_max,
                                     double* d_corr_lo, double* d_corr_hi, double* d_clearance);

/* BASELINE config 5 as ONE call (north-star extension: "SE(3) ellipsoid-collision corridor + time-reallocation outer loop"; the
 * reference has no such loop -- constant 1.0 s per segment, test_minimum_jerk.cpp:65-71, every row an equality,
 * minimum_control.cpp:98-125 -- so parity is per inner solve, SURVEY.md section 8-a').  Host-side C++ sequencing of the entry points
 * above on device buffers:
 *   uavqp_solve_batch_device (the reference's equality problem) -> uavqp_corridor_from_cloud_device (boxes, attitude of that solve)
 *   -> at most max_rounds x (uavqp_solve_corridor_warm_device -- from the second round on warm_start = 2: working set carried over, previous
 *   polynomials as the starting point -- + uavqp_time_reallocate_device; the loop ends
 *   as soon as a re-allocation stretches nothing; if the cap is reached with durations still changing, one more solve makes the
 *   coefficients match d_times) -> uavqp_ellipsoid_check_grid_device on check_samples samples per trajectory (ONE time grid for the
 *   batch: dt = longest total duration / (check_samples - 1)) -> at most repair_rounds x (the boxes of every colliding trajectory
 *   are halved towards its waypoints -- in the last repair round collapsed onto them: the reference's equality rows --, warm re-solve,
 *   one re-allocation, re-solve if that stretched anything, check again).  A colliding trajectory with an interior waypoint whose box
 *   is degenerate (the cloud leaves no room around the searcher's waypoint) cannot be helped by narrower boxes: counted, not repaired.
 * Loop control is data dependent: the number of trajectories a round stretched reaches the host through a word of pinned,
 * host-coherent memory that the round's last kernel writes and the host polls (no copy, no event, no stream stop between rounds; round
 * 1, and later rounds while they still stretch more than n_traj / 64 trajectories, are enqueued before the previous count is looked
 * at, and so is the extra solve at the cap -- a round that turns out to be unnecessary works on an empty list and changes no byte).  From the second round on, re-allocation and compaction only visit the trajectories the previous
 * round re-solved.  The check needs no host round trip of its own: the longest duration stays on the device (the check kernel forms dt
 * from it), and ONE counter block read after the check carries hits, blocked waypoints, unsolved trajectories and that duration; the
 * call returns with the stream idle (SYNCHRONOUS).  The check itself does not test samples beyond a trajectory's end more than once
 * (they all are its end point and could only repeat the first one's verdict at a larger index).
 *   total_segments      sum_b M_b (the host knows it: it sized the buffers); uniform batches: n_traj * uniform_segments
 *   d_times             [total_segments] IN / OUT: stretched in place by the re-allocation (never shrunk)
 *   grid                uniform grid over d_obstacles with cell = check radius + 0.1 (uavqp_obstacle_grid_build_device), or NULL: built
 *                       and destroyed inside the call (a planner builds it once per map)
 *   d_corr_lo / d_corr_hi [total_segments + n_traj][3] OUT: the boxes of the final solve
 *   d_first_hit         [n_traj] OUT (may be NULL): first colliding sample of the final check, check_samples = collision-free
 *   params              uavqp_default_pipeline_params fills the launch-file values of the reference's kino-A* test
 *                       (test_kino_astar_searching.launch:49-57: robot 0.4 x 0.1 m, 7 m/s, 10 m/s^2); check_samples = 0 skips
 *                       the check and the repair; check_robot_r / _h > 0 check with another ellipsoid than the boxes were built with
 *   result              (may be NULL) rounds run, repair rounds run, trajectories still stretching at the cap, colliding at the first
 *                       check / of those with a blocked waypoint / colliding at the last check, trajectories not UAVQP_SOLVED, rows
 *                       placed and kept by a rows repair (0 from this entry point), the dt of the check grid. */
typedef struct uavqp_pipeline_params {
    int32_t struct_size;
    int32_t max_rounds;
    double robot_r, robot_h, h_max;
    double v_max, a_max;
    int32_t samples_per_seg;
    int32_t check_samples;
    double max_stretch;
    int32_t repair_rounds;
    int32_t reserved_;
    double check_robot_r, check_robot_h;
} uavqp_pipeline_params;
typedef struct uavqp_pipeline_result {
    int32_t rounds, repairs, still_stretching, colliding_before_repair, colliding_with_blocked_waypoints, colliding_after, unsolved, repair_rows;
    double check_dt;
} uavqp_pipeline_result;
void uavqp_default_pipeline_params(uavqp_pipeline_params* out);
int uavqp_corridor_pipeline_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                   const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                   const double* d_obstacles, int n_obs, const uavqp_grid* grid, const uavqp_pipeline_params* params,
                                   double* d_coeff_out, int32_t* d_status_out, double* d_corr_lo, double* d_corr_hi,
                                   int32_t* d_first_hit, uavqp_pipeline_result* result);
/* The same from HOST pointers (staged through device memory; times is updated in place; corr_lo / corr_hi / first_hit may be NULL):
 * what a C++ planner that keeps its paths in host memory calls -- TrajOptimizer::solvePipeline. */
int uavqp_corridor_pipeline_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                 const double* waypoints, double* times, const double* bc, const double* obstacles, int n_obs,
                                 const uavqp_pipeline_params* params, double* coeff_out, int32_t* status_out, double* corr_lo,
                                 double* corr_hi, int32_t* first_hit, uavqp_pipeline_result* result);

/* Rows repair of the pipeline: between-knot collisions become position rows instead of shrunken boxes.
 * uavqp_repair_rows_from_hits_device -- rows from the per-sample verdicts of a check (d_flags [n_traj][n_samples] uint8, the samples
 *   t_s = t0 + s dt of uavqp_ellipsoid_check_device, segment rule of uavqp_eval_batch_device).  For every segment i with colliding samples:
 *   s = middle sample of the first colliding run in it, tau = (t_s - t_start_i) / T_i clamped to [1/32, 31/32]; attitude from the
 *   polynomials' acceleration at t_s (b3 = normalize(acc + 9.81 z), the frame of uavqp_corridor_from_cloud_device), E = Rot diag(robot_r,
 *   robot_r, robot_h) Rot'; anchor a = p(t_s) pushed out of the cloud: while g(a) = min over ALL points o of |E^-1 (o - a)| is below
 *   G = 2, at most 4 times, a <- o* + (a - o*) G / g(a) with o* the arg-min point.  If g(a) > 1 at the end the segment gets the row
 *   a - h <= p_i(tau T_i) <= a + h, h_k = min(h_max, (g(a) - 1) / (3 |E^-1 e_k|)) (the guarantee of the knot boxes: the robot ellipsoid
 *   anywhere in the row's box holds no point), derivative 0 -- in slot 0, or in slot 1 when slot 0 is taken and |tau - tau_0| > 1/32;
 *   both taken: no row.  d_waypoints is the batch's [sum(M+1)][3] (checked, not read).
 *   d_row_tau / d_row_deriv / d_row_lo / d_row_hi  IN / OUT, the rows_per_segment = 2 layout of uavqp_solve_rows_batch_device
 *   d_new_rows   [n_traj] int32 OUT: rows placed by this call.  Asynchronous on the ctx stream.
 * uavqp_corridor_pipeline_rows_device / _host -- uavqp_corridor_pipeline_* with the rows repair in place of the box repair (arguments
 *   of those plus the caller's row arrays [total_segments][2] (tau, deriv) / [total_segments][2][3] (lo, hi): set to unused (deriv -1)
 *   by the call, on return the rows of the final solve).  A repair round: the check also writes its per-sample verdicts, the rows above
 *   are placed for every colliding trajectory (blocked waypoints included; not for M = 1 or M > 63) with the CHECK's ellipsoid, the
 *   trajectories that got one are gathered into a ragged sub-batch (one row per segment when none uses slot 1) and solved by
 *   uavqp_solve_rows_batch_device with their knot boxes and all their rows; one time re-allocation of the sub-batch and, if it stretched
 *   anything, a second rows solve (rows are fractions of T_i: they stay attached); what ended UAVQP_SOLVED is written back, the others keep
 *   coefficients, durations and status and lose the rows of that round.  Knot boxes never change, trajectories never flagged are not
 *   touched: their output is the repair_rounds = 0 output bit for bit.  result->repair_rows = rows in place on return. */
int uavqp_repair_rows_from_hits_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                       const double* d_waypoints, const double* d_times, const double* d_coeff, int n_samples, double t0,
                                       double dt, const uint8_t* d_flags, const double* d_obstacles, int n_obs, double robot_r,
                                       double robot_h, double h_max, double* d_row_tau, int32_t* d_row_deriv, double* d_row_lo,
                                       double* d_row_hi, int32_t* d_new_rows);
int uavqp_corridor_pipeline_rows_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                        const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                        const double* d_obstacles, int n_obs, const uavqp_grid* grid, const uavqp_pipeline_params* params,
                                        double* d_coeff_out, int32_t* d_status_out, double* d_corr_lo, double* d_corr_hi,
                                        int32_t* d_first_hit, double* d_row_tau, int32_t* d_row_deriv, double* d_row_lo,
                                        double* d_row_hi, uavqp_pipeline_result* result);
int uavqp_corridor_pipeline_rows_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                      const double* waypoints, double* times, const double* bc, const double* obstacles, int n_obs,
                                      const uavqp_pipeline_params* params, double* coeff_out, int32_t* status_out, double* corr_lo,
                                      double* corr_hi, int32_t* first_hit, double* row_tau, int32_t* row_deriv, double* row_lo,
                                      double* row_hi, uavqp_pipeline_result* result);

/* quadrotor_msgs/PolynomialTrajectory packer.  HOST function, no ctx, no device: turns ONE solved
 * trajectory (the [axis][segment][2r] slice of coeff_out that belongs to it) into the arrays of the message the rest of the
 * reference stack consumes -- src/simulator/utils/quadrotor_msgs/msg/PolynomialTrajectory.msg:1-28; the only consumer in the
 * reference is trajCallback, src/planner/traj_server/src/poly_traj_server.cpp:57-81, which reads num_order + 1 coefficients per
 * segment and axis from coef_x / coef_y / coef_z (ascending powers, segment-local time: the layout of coef_1d_,
 * minimum_control.cpp:186) and the segment durations from time[].  Nobody in the reference PRODUCES this message; this closes
 * the loop from the solver to poly_traj_server.
 *   coeff_traj  [3][n_seg][2r]   one trajectory of uavqp_solve_*'s coeff_out
 *   times       [n_seg]
 *   coef_x / coef_y / coef_z [n_seg * 2r], time_out [n_seg], order_out [n_seg] (uint32, = 2r - 1 each): caller-allocated
 *   num_order_out = 2r - 1, num_segment_out = n_seg (the message's scalar fields; trajectory_id, action = ACTION_ADD (1),
 *   start_yaw / final_yaw, mag_coeff, header.stamp are the caller's).
 * Returns UAVQP_ERR_INVALID_ARG for r not in {3, 4}, n_seg < 1, a null pointer, or a non-positive / non-finite duration
 * (poly_traj_server would walk off the end of such a trajectory). */
int uavqp_pack_polynomial_trajectory(int r, int n_seg, const double* coeff_traj, const double* times, double* coef_x, double* coef_y,
                                     double* coef_z, double* time_out, uint32_t* order_out, uint32_t* num_order_out,
                                     uint32_t* num_segment_out);

/* ---- Multi-GPU: contiguous shards of the batch, one process (or thread) and one ctx per GPU ----
 * Trajectories are independent QPs, so the solve itself needs no collective: every rank solves its own slice with the entry
 * points above.  The one exchange step is the all-gather of the solved coefficient shards over xGMI (RCCL).  The reference has
 * no multi-device code (its only remark on parallelism: test_minimum_jerk.cpp:73-74); nothing to mirror.
 *
 *   uavqp_shard_bounds          bounds[g] = floor(n_traj g / world), g = 0..world: rank g owns trajectories [bounds[g], bounds[g+1]).
 *   uavqp_shard_bounds_ragged   same, balanced by total SEGMENT count (work is proportional to M_b): bounds[g] is the first
 *                               trajectory whose segment offset reaches g / world of the total.  Host arithmetic on the host CSR
 *                               offsets; no device, no communicator.
 *   uavqp_comm_unique_id        fills a UAVQP_UNIQUE_ID_BYTES token on ONE rank (RCCL's ncclGetUniqueId); the caller ships it to
 *                               the other ranks by whatever it has (MPI, a file, a socket, torch.distributed's store).
 *   uavqp_comm_create           collective over all ranks: the ctx creates and owns the RCCL communicator (one per ctx; released
 *                               by uavqp_comm_destroy / uavqp_destroy).  world = 1 is valid (single-GPU self test).
 *   uavqp_comm_info             rank and world size of the ctx's communicator as RCCL reports them (ncclCommUserRank, ncclCommCount):
 *                               what bench.py records as allgather.rccl_world -- evidence that the exchange ran on a communicator of N ranks.
 *   uavqp_allgather_coeffs      device buffers, asynchronous on the ctx stream (ordered behind the solve): rank g contributes
 *                               counts[g] doubles from d_local; d_full receives the shards back to back in rank order
 *                               (sum_g counts[g] doubles).  Equal counts: one ncclAllGather; otherwise every rank sends its shard
 *                               to every peer directly (grouped ncclSend / ncclRecv: one hop per peer on the xGMI full mesh, no
 *                               padding).  d_local may alias its own slot of d_full (in place).
 *   uavqp_allgather_status      the same for the int32 status arrays (counts in trajectories).
 * RCCL is bound at run time (librccl.so.1); without it uavqp_comm_* return UAVQP_ERR_RCCL and uavqp_last_error() says why. */
#define UAVQP_UNIQUE_ID_BYTES 128
int uavqp_shard_bounds(int n_traj, int world, int32_t* bounds);
int uavqp_shard_bounds_ragged(const int32_t* seg_offsets, int n_traj, int world, int32_t* bounds);
int uavqp_comm_unique_id(void* id_out);
int uavqp_comm_create(uavqp_ctx* ctx, int rank, int world, const void* unique_id);
int uavqp_comm_info(const uavqp_ctx* ctx, int32_t* rank_out, int32_t* world_out);
int uavqp_comm_destroy(uavqp_ctx* ctx);
int uavqp_allgather_coeffs(uavqp_ctx* ctx, const double* d_local, const int64_t* counts, double* d_full);
int uavqp_allgather_status(uavqp_ctx* ctx, const int32_t* d_local, const int64_t* counts, int32_t* d_full);

/* hipGraph capture of a launch-bound inner loop: everything enqueued on the ctx stream between
 * uavqp_capture_begin and uavqp_capture_end (any number of uavqp_solve_batch_device calls with their
 * workspaces already sized by one eager call) becomes one executable graph; uavqp_graph_launch replays
 * it on the ctx stream.  No reference counterpart (the reference has no device queue).
 *
 * A replay may run captured solves CONCURRENTLY.  uavqp_capture_end knows which bytes every captured uniform-batch
 * uavqp_solve_batch_device call reads (waypoints, times, bc) and writes (coeff_out, status_out) and orders two of them only
 * where those ranges overlap (read after write, write after read, write after write); solves on disjoint buffers become
 * chain graphs on streams of the ctx ("lanes"), forked from and joined to the ctx stream by events (work queued on the ctx stream
 * behind uavqp_graph_launch waits for all of it): at most UAVQP_CAPTURE_LANES (default 4, 1..8; 1 = keep the captured order) side
 * by side, and a lane only where there are 16 launches for it (UAVQP_CAPTURE_LANE_NODES) -- a shorter capture replays as captured.
 * When a replay completes, every buffer holds what the calls would have left in the order they were captured.  One visible
 * difference: a status store that a LATER captured solve overwrites completely, with nothing in between touching those
 * entries, is not performed (that is what lets steps that share one status array overlap) -- the array holds the last
 * writer's codes, as in serial order, but never an earlier solve's codes in the meantime.
 * Ragged batches, and batches that take a kernel with a ctx workspace, are ordered against everything before and after them.
 * A capture that contains anything else -- another entry point's launch, a copy, a foreign node -- and a process started
 * with GPU_MAX_HW_QUEUES below 4 (read, never set) replay exactly the chain that was captured. */
int uavqp_capture_begin(uavqp_ctx* ctx);
int uavqp_capture_end(uavqp_ctx* ctx, void** out_graph_exec);   /* the handle is the library's own: only for uavqp_graph_launch / _destroy */
int uavqp_graph_launch(uavqp_ctx* ctx, void* graph_exec);
int uavqp_graph_destroy(uavqp_ctx* ctx, void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* UAVQP_H_ */
