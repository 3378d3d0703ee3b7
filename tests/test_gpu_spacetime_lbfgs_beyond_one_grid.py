"""-m gpu: uavqp_spacetime_lbfgs_device on more trajectories than one launch of the step kernel holds, in the pattern of
test_optimiser_past_one_grid_equals_separate_calls (tests/test_gpu_beyond_one_grid.py, whose tiled batch and scene it imports).

topt_grid() caps a launch at 32 x (number of CUs) blocks of 8 trajectories; beyond 8 x 32 x CUs trajectories a lane group takes a second
trajectory in the same launch (the stride round).  Everything the step keeps between launches -- the best point and its gradient, the
history slots, head / count / mode / rejections, alpha, the scales -- is indexed by trajectory, so ONE call on n = 8 x 32 x CUs + 24
trajectories must give the bytes of TWO calls that fit one grid each.  max_iters = 4, memory = 2: the ring of three slots wraps, pairs
are dropped, and with durations that differ between the copies some trials are rejected.  The designed invalid trajectory sits in the
stride round."""
import numpy as np
import pytest

import esdf_scene as S
import spacetime_reference as R
import test_gpu_beyond_one_grid as B
import uav_motion_planning_amd as U

pytestmark = pytest.mark.gpu
ITERS, MEMORY = 4, 2
KEYS = ("wp", "T", "coeff", "status", "obj", "acc", "peak", "md", "outside")


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    m, ref_dist = S.build_scene(gpu_ctx)
    yield m, ref_dist
    m.close()


def run(w, esdf, lo, hi):
    torch, d = B.dev()
    n, total, d_so, d_wp, d_T, d_bc = w.part(lo, hi)
    z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=d)
    o = dict(coeff=z(w.nc3 * total), status=z(n, dtype=torch.int32), obj=z(n, 2), acc=z(n, dtype=torch.int32), peak=z(n, 2), md=z(n),
             outside=z(n, dtype=torch.int32))
    torch.cuda.synchronize()
    w.ctx.spacetime_lbfgs_device(w.r, n, 0, 3, total, d_so, d_wp, d_T, d_bc, esdf, o["coeff"], o["status"], o["obj"], o["acc"], o["peak"], o["md"],
                                 o["outside"], limits=R.LIMITS_OF[w.r], clearance=R.CLEARANCE, max_iters=ITERS, memory=MEMORY, max_move=1.0)
    w.ctx.synchronize()
    o["T"], o["wp"] = d_T, d_wp
    return {k: o[k] for k in KEYS}


def test_lbfgs_past_one_grid_equals_separate_calls(gpu_ctx, scene):
    torch, _ = B.dev()
    m, _ = scene
    if 3 not in B._whole:
        B._whole[3] = B.Whole(gpu_ctx, 3)
    w = B._whole[3]
    whole = run(w, m, 0, w.n)
    so, cut, n = w.so, w.cut, w.n
    assert n == B.one_grid() + 24
    for lo, hi in ((0, cut), (cut, n)):
        part = run(w, m, lo, hi)
        s0, s1 = int(so[lo]), int(so[hi])
        span = dict(traj=(lo, hi), seg=(s0, s1), row=(s0 + lo, s1 + hi), coeff=(w.nc3 * s0, w.nc3 * s1))
        for k, v in part.items():
            a, b = span[B.SPLIT_KEYS[k]]
            assert torch.equal(B.bits(whole[k][a:b].contiguous()), B.bits(v)), f"{k} of trajectories {lo} .. {hi} differs between one call and two"
    # the stride round did something: the invalid trajectory is refused, the others moved, and not every trial was accepted
    tail = np.arange(B.one_grid(), n)
    st, acc = whole["status"].cpu().numpy(), whole["acc"].cpu().numpy()
    bad = B.one_grid() + 5
    assert st[bad] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st[tail], 5) == U.UAVQP_SOLVED) and acc[bad] == 0
    assert np.all(np.isnan(whole["obj"].cpu().numpy()[bad]))
    moved = np.add.reduceat(whole["T"].cpu().numpy() != w.T_start, so[:-1]) > 0
    moved |= np.add.reduceat(np.any(whole["wp"].cpu().numpy() != w.wp_start, axis=1), so[:-1] + np.arange(n)) > 0
    assert not moved[bad]
    valid = np.delete(tail, 5)
    rejected = np.count_nonzero((acc[valid] < ITERS) & moved[valid])
    rejected_all = np.count_nonzero((acc < ITERS) & moved)
    print(f"lbfgs: {rejected_all} of {n} moved and were rejected at least once")
    print(f"lbfgs: {n} trajectories in one call = {cut} + {n - cut} in two, bytes equal; stride round: {np.count_nonzero(moved[tail])} of {tail.size} "
          f"moved, accepted trials {acc[valid].min()} .. {acc[valid].max()} of {ITERS}, {rejected} moved and were rejected at least once; all: "
          f"{np.count_nonzero(acc == ITERS)} accepted every trial (the ring of {MEMORY + 1} slots wrapped)")
    assert np.count_nonzero(moved[tail]) * 20 >= tail.size
    # (four trials: a rejection need not fall into the 23 valid trajectories of the stride round; both parts of the batch see some)
    assert rejected_all >= 1 and np.count_nonzero((acc[cut:] < ITERS) & moved[cut:]) >= 1 and np.count_nonzero(acc[valid] > 0) >= 1
    assert np.count_nonzero(acc == ITERS) >= 1
    # the copies differ in their start, and so in their course
    first = np.flatnonzero(w.src == int(w.src[valid[0]]))
    assert len({int(a) for a in acc[first]}) > 1 or len({x.tobytes() for x in whole["obj"].cpu().numpy()[first]}) > 10
