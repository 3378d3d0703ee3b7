// uavqp_solved.h -- what the entries of include/uavqp.h that EVALUATE a batch of solved trajectories share (included by uavqp.hip behind
// uavqp_stage.h): the limit, clearance, flight, attitude, swarm and moving-obstacle penalties, the envelope and the clearance,
// separation and moving-obstacle certificates, each as a _device and a _host entry.  One description of the batch (SolvedBatch), one argument check, one
// staging of its four arrays, one fill of the kernel arguments, one alignment test, one dispatch of the kernel's template arguments.
// Host only; everything but the dispatch is plain C++ and compiles without the HIP runtime (tests/cpp/test_solved_args.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

// (r, n_traj, uniform_segments, seg_offsets, times, coeff, status) as every such entry takes them: host pointers in a _host entry before
// staging, device pointers everywhere else.  Built once at the top of an entry and handed on by reference.
struct SolvedBatch {
    int r, n_traj, uniform;
    const int32_t* seg_offsets;
    const double* times;
    const double* coeff;
    const int32_t* status;
};

// The swarms of the swarm entries: trajectories offsets[g] .. offsets[g + 1]; offsets null: the whole batch is ONE swarm.
struct SolvedGroups {
    int n_groups;
    const int32_t* offsets;
};

// The refusal precedence of the twenty entries, in this order; everything refused is UAVQP_ERR_INVALID_ARG and nothing is touched.
// groups null: the PER-TRAJECTORY rule; groups given: the SWARM rule.
//   1. ctx, r (3 or 4) and the counts: n_traj, uniform_segments and (SWARM) n_groups must not be negative;
//   2. params_ok(), called only behind 1: the entry's parameter structs and its own preconditions (the distance field of the map
//      entries, the obstacle struct of the moving penalty and certificate, "both boxes or neither" of the envelope) -- so a bad struct is refused
//      even where there is nothing to do;
//   3. SWARM only: without offsets n_groups must be 1 -- refused even where no output is asked for;
//   4. nothing to do: UAVQP_OK, *run stays false.  PER-TRAJECTORY: n_traj == 0 or no output asked for.  SWARM: n_groups == 0 or no
//      output asked for -- an empty n_traj with swarms left is a call like any other (each swarm's penalty is written);
//   5. a missing array: times, coeff, and seg_offsets when ragged -- needed only where n_traj > 0, which 4 has made sure of for
//      PER-TRAJECTORY.
// *run: the entry goes on (hipSetDevice, what its _host form checks inside the arrays, the launch).
template <class ParamsOk>
static int solved_args_check(const uavqp_ctx* ctx, const SolvedBatch& B, ParamsOk&& params_ok, bool any_output, bool* run,
                             const SolvedGroups* groups = nullptr) {
    *run = false;
    if (!ctx || (B.r != 3 && B.r != 4) || B.n_traj < 0 || B.uniform < 0 || (groups && groups->n_groups < 0)) return UAVQP_ERR_INVALID_ARG;
    if (!params_ok()) return UAVQP_ERR_INVALID_ARG;
    if (groups && !groups->offsets && groups->n_groups != 1) return UAVQP_ERR_INVALID_ARG;
    if ((groups ? groups->n_groups == 0 : B.n_traj == 0) || !any_output) return UAVQP_OK;
    if (B.n_traj > 0 && (!B.times || !B.coeff || (B.uniform == 0 && !B.seg_offsets))) return UAVQP_ERR_INVALID_ARG;
    *run = true;
    return UAVQP_OK;
}

// batch_shape of a batch that passed the check (no trajectory, which only the swarm entries get this far with: no segment)
static inline int solved_shape(const SolvedBatch& B, BatchShape* sh) {
    *sh = BatchShape{0, 1};
    return B.n_traj > 0 ? batch_shape(B.n_traj, B.uniform, 0, B.seg_offsets, sh) : UAVQP_OK;
}

// The four arrays of a _host entry on its Stage: declare() before stage_begin and before anything else the entry declares, device()
// behind it gives the batch the device side takes.  The ORDER offsets, times, coeff, status is part of the contract: the carver places
// slots in declaration order, so it fixes every device address behind it and with them the 16-byte alignment the kernels test.
struct SolvedStage {
    SolvedBatch b;
    int off, t, c, s;
    void declare(Stage& stage, const SolvedBatch& B, const BatchShape& sh) {
        const size_t n = (size_t)B.n_traj, tot = (size_t)sh.total_seg;
        b = B;
        off = (B.uniform > 0 || B.n_traj == 0) ? -1 : stage.in(B.seg_offsets, sizeof(int32_t) * (n + 1));
        t = stage.in(B.times, sizeof(double) * tot);
        c = stage.in(B.coeff, sizeof(double) * 3 * 2 * B.r * tot);
        s = B.status ? stage.in(B.status, sizeof(int32_t) * n) : -1;
    }
    SolvedBatch device(const Stage& stage) const {
        return SolvedBatch{b.r, b.n_traj, b.uniform, stage.at<int32_t>(off), stage.at<double>(t), stage.at<double>(c), stage.at<int32_t>(s)};
    }
};

// the six fields every kernel argument struct of these families names alike
template <class Args>
static inline void solved_fill(Args& a, const SolvedBatch& B) {
    a.n_traj = B.n_traj; a.uniform = B.uniform; a.seg_offsets = B.seg_offsets; a.times = B.times; a.coeff = B.coeff; a.status = B.status;
}

// al16 of the sampling kernels: coefficients and their gradient (null counts as aligned) may be read and written two doubles at a time
static inline int coeff_al16(const double* coeff, const double* grad_coeff) {
    return ((((uintptr_t)coeff) | ((uintptr_t)grad_coeff)) & 15u) == 0 ? 1 : 0;
}

#ifdef UAVQP_HIP
// The dispatch of a kernel template on <R> and on <R, FLAG> -- FLAG: INIT of a descent step, ACC of an accumulating penalty -- and the
// error of its launch.  launch gets the template arguments as integral constants and names its kernel with decltype(R)::value,
// decltype(FLAG)::value (and whatever further template arguments it has).
template <class Launch>
static int dispatch_r(int r, Launch&& launch) {
    if (r == 3) launch(std::integral_constant<int, 3>{});
    else launch(std::integral_constant<int, 4>{});
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}
template <class Launch>
static int dispatch_r_flag(int r, bool flag, Launch&& launch) {
    return dispatch_r(r, [&](auto R) {
        if (flag) launch(R, std::true_type{});
        else launch(R, std::false_type{});
    });
}
#endif
