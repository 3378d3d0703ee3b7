"""-m gpu: the eight-lanes-per-trajectory kernels, the field query and the rasteriser with more work than one launch holds.

topt_grid() caps a launch at 32 x (number of CUs) blocks of 8 trajectories; beyond 8 x 32 x CUs trajectories a lane group takes a second
trajectory in the same launch (the stride round).  The query and the rasteriser cap theirs at 32 x CUs blocks of 256 lanes.

Evaluation entries (cost / time gradient, limit, clearance and flight penalty, cost / waypoint gradient).  61 distinct trajectories of
1 .. 3 segments (tests/esdf_scene.py: base_flight_batch) are solved once and tiled on the device to n = 8 x 32 x CUs + 11 by index % 61:
61 is odd, so the copies of one trajectory sit on different sub-lane groups and in different blocks.  One trajectory has an invalid
duration -- the one whose copy falls into the stride round.  The first 61 results are compared with the high-precision reference of the
entry's own test at that test's tolerance; every later copy must have the BYTES of its base trajectory: these kernels read given
coefficients and durations and run no solve, and nothing in a trajectory's arithmetic depends on where it sits (the 16-byte path of the
coefficient loads is chosen per call, and 3 x 2r x s0 doubles is a multiple of 16 bytes for every s0).

Optimisers.  One call on n = 8 x 32 x CUs + 24 trajectories against the same data as two calls that fit one grid each, byte for byte
(the pattern of test_grid_stride_rounds_equal_separate_launches, tests/test_gpu_solve_backward.py).  The inner solve is chosen from
n_traj: for a ragged batch whose longest trajectory has 3 segments it is the two-lanes-per-trajectory kernel at every size (Mmax >= 3 and
16-byte aligned arrays select it whatever n_traj is; its waves per CU do not depend on n_traj), with the dealing by segment count inside
windows of 512 trajectories from 2048 trajectories on.  Both parts hold at least 2048 trajectories and the cut is a multiple of 512, so
whole and parts run the same kernel with the same windows; the parts are copied into allocations of their own, so they are 16-byte
aligned like the whole.  The backward pass inside three of the optimisers is one kernel with one lane per trajectory at every size; only
its grid is capped (at 128 x CUs trajectories, so it strides in the whole and in the second part alike)."""
import numpy as np
import pytest

import esdf_reference as E
import esdf_scene as S
import limit_penalty_reference as L
import spacetime_reference as R
import uav_motion_planning_amd as U
from uav_motion_planning_amd.esdf import EsdfMap

pytestmark = pytest.mark.gpu
LD = np.longdouble
PARITY = 1e-9          # tests/test_gpu_limit_penalty.py, tests/test_gpu_esdf.py, tests/test_gpu_spacetime.py
NB = S.BASE_N


def dev():
    import torch
    return torch, torch.device("cuda", 0)


def cus():
    torch, _ = dev()
    return torch.cuda.get_device_properties(0).multi_processor_count


def one_grid():
    """the most trajectories one launch of an eight-lanes-per-trajectory kernel takes without striding"""
    return 8 * 32 * cus()


def up(x):
    torch, d = dev()
    return torch.from_numpy(np.ascontiguousarray(x)).to(d)


def bits(x):
    """a float64 / int32 / uint8 tensor as integers: NaN compares equal to itself"""
    torch, _ = dev()
    return x.view(torch.int64) if x.dtype == torch.float64 else x


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    m, ref_dist = S.build_scene(gpu_ctx)
    yield m, ref_dist
    m.close()


class Tiled:
    """the base batch solved once on the device, and its inputs, coefficients and statuses tiled to n trajectories by index % 61"""

    def __init__(self, ctx, r, n):
        torch, d = dev()
        self.ctx, self.r, self.n, self.nc3 = ctx, r, n, 3 * 2 * r
        self.bad = (one_grid() + 5) % NB                   # its copy one_grid() + 5 lies in the stride round
        b = self.b = S.base_flight_batch(r, bad=self.bad)
        so0, Ms0 = b["so"].astype(np.int64), np.diff(b["so"]).astype(np.int64)
        self.total0 = int(so0[-1])
        # the small call
        self.coeff0 = torch.zeros(self.nc3 * self.total0, dtype=torch.float64, device=d)
        self.status0 = torch.zeros(NB, dtype=torch.int32, device=d)
        torch.cuda.synchronize()
        ctx.solve_batch_device(r, NB, 0, 3, up(b["so"]), up(b["wp"]), up(b["T_bad"]), up(b["bc"]), self.coeff0, self.status0)
        ctx.synchronize()
        st = self.status0.cpu().numpy()
        assert st[self.bad] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st, self.bad) == U.UAVQP_SOLVED)
        # trajectory t is a copy of t % 61; the index arrays below gather per trajectory, per segment, per waypoint row, per coefficient
        self.src = np.arange(n, dtype=np.int64) % NB
        Ms = Ms0[self.src]
        so = np.zeros(n + 1, dtype=np.int64)
        so[1:] = np.cumsum(Ms)
        self.so, self.Ms, self.total = so, Ms, int(so[-1])
        assert np.array_equal(so[:NB + 1], so0)            # the first 61 are the base batch itself
        shift = so0[self.src] - so[:-1]                    # base segment index - segment index, per trajectory
        self.i_traj = up(self.src)
        self.i_seg = up(np.repeat(shift, Ms) + np.arange(self.total))
        self.i_row = up(np.repeat(shift + self.src - np.arange(n), Ms + 1) + np.arange(self.total + n))
        self.i_coeff = up(np.repeat(self.nc3 * shift, self.nc3 * Ms) + np.arange(self.nc3 * self.total))
        self.d_so = up(so.astype(np.int32))
        self.d_T = up(b["T_bad"])[self.i_seg]
        self.d_wp = up(b["wp"])[self.i_row]
        self.d_bc = up(b["bc"])[self.i_traj]
        self.coeff = self.coeff0[self.i_coeff]
        self.status = self.status0[self.i_traj]
        self.index = dict(traj=self.i_traj, seg=self.i_seg, row=self.i_row, coeff=self.i_coeff)
        self.ok = np.arange(NB) != self.bad

    def out(self, kind, cols=None, dtype=None):
        """a sentinel-filled output with one entry (or `cols`) per trajectory / segment / waypoint row / coefficient"""
        torch, d = dev()
        rows = dict(traj=self.n, seg=self.total, row=self.total + self.n, coeff=self.nc3 * self.total)[kind]
        shape = (rows,) if cols is None else (rows, cols)
        return torch.full(shape, -7, dtype=dtype, device=d) if dtype is not None else torch.full(shape, float("nan"), dtype=torch.float64, device=d)

    def copies_equal_the_base(self, x, kind, what):
        """every trajectory's part of x has the bytes of its base trajectory's part (the first 61 trajectories of x itself)"""
        torch, _ = dev()
        b = bits(x)
        assert torch.equal(b, b[self.index[kind]]), f"{what}: a copy differs from its base trajectory"
        return x.cpu().numpy()

    def unsolved_is_zero(self, x, kind, what):
        """the invalid trajectory's copies hold zero bytes -- the one of the stride round among them"""
        t = one_grid() + 5
        assert t < self.n and t % NB == self.bad
        s0, M = int(self.so[t]), int(self.Ms[t])
        lo, hi = dict(traj=(t, t + 1), seg=(s0, s0 + M), row=(s0 + t, s0 + M + t + 1), coeff=(self.nc3 * s0, self.nc3 * (s0 + M)))[kind]
        part = x[lo:hi]
        assert part.size > 0 and part.tobytes() == bytes(part.nbytes), f"{what}: the unsolved trajectory of the stride round is not zero"


def worst_errors(so, r, got, ref, keys):
    """max |got - ref| relative to the per-trajectory largest magnitude of ref, per output, over the base trajectories"""
    nc3 = 3 * 2 * r
    worst = {}
    for t in range(NB):
        s0, s1 = int(so[t]), int(so[t + 1])
        sl = dict(phi=slice(t, t + 1), grad_coeff=slice(nc3 * s0, nc3 * s1), grad_times=slice(s0, s1), peak=t, min_dist=slice(t, t + 1))
        for key in keys:
            want = np.atleast_1d(ref[key][sl[key]]).astype(LD)
            have = np.atleast_1d(got[key][sl[key]]).astype(LD)
            scale = np.max(np.abs(want))
            err = float(np.max(np.abs(have - want)) / scale) if scale > 0 else float(np.max(np.abs(have)))
            worst[key] = max(worst.get(key, 0.0), err)
    return worst


_tiled = {}


def tiled(gpu_ctx, r):
    if r not in _tiled:
        _tiled[r] = Tiled(gpu_ctx, r, one_grid() + 11)
    return _tiled[r]


# ---------------------------------------------------------------------------------------------------------------- evaluation entries
def test_tiled_batch_goes_past_one_grid(gpu_ctx):
    t = tiled(gpu_ctx, 3)
    assert t.n * 8 > 64 * 32 * cus() and t.n - one_grid() == 11
    assert len({int(k) % 8 for k in np.flatnonzero(t.src == 0)[:8]}) == 8      # the copies of one trajectory: every lane group of a wave


def test_cost_time_gradient_past_one_grid(gpu_ctx, oracle):
    """cost 1e-9 relative to the oracle's; the gradient within 10 x the central-difference scheme's own error (h against h / 2), which
    must stay under 1e-5 -- the bounds of tests/test_gpu_time_opt.py.  The entry takes no status: the unsolved trajectory's copies are
    only compared with each other."""
    t = tiled(gpu_ctx, 3)
    r, b = t.r, t.b
    cost, grad = t.out("traj"), t.out("seg")
    gpu_ctx.cost_time_gradient_device(r, t.n, 0, t.d_so, t.d_T, t.coeff, cost, grad)
    gpu_ctx.synchronize()
    cost, grad = t.copies_equal_the_base(cost, "traj", "cost"), t.copies_equal_the_base(grad, "seg", "grad")
    H_REL, worst_cost, worst_err, worst_rich = 1e-4, 0.0, 0.0, 0.0
    for k in np.flatnonzero(t.ok):
        s0, s1 = int(b["so"][k]), int(b["so"][k + 1])
        w_k, bc_k, T_k, M = b["wp"][s0 + k:s1 + k + 1], b["bc"][k], b["T"][s0:s1], s1 - s0

        def J(T):
            return sum(2.0 * oracle.cost(r, T, oracle.solve_exact(r, w_k[:, ax], bc_k[0, :, ax], bc_k[1, :, ax], T)) for ax in range(3))

        def fd(h):
            g = np.zeros(M)
            for i in range(M):
                e = np.zeros(M)
                e[i] = h * T_k[i]
                g[i] = (J(T_k + e) - J(T_k - e)) / (2.0 * e[i])
            return g
        want = J(T_k)
        worst_cost = max(worst_cost, abs(cost[k] - want) / want)
        g1, g2 = fd(H_REL), fd(H_REL / 2)
        scale = np.max(np.abs(g2))
        worst_rich = max(worst_rich, np.max(np.abs(g1 - g2)) / scale)
        worst_err = max(worst_err, np.max(np.abs(grad[s0:s1] - g2)) / scale)
    print(f"cost / time gradient, {t.n} trajectories: copies bytes equal; cost rel err {worst_cost:.3e}; |grad - central difference| / max|grad| "
          f"{worst_err:.3e}, the scheme's own error {worst_rich:.3e}")
    assert worst_cost <= 1e-9
    assert worst_rich < 1e-5, "the finite-difference step is badly chosen"
    assert worst_err <= 10.0 * worst_rich


def test_limit_penalty_past_one_grid(gpu_ctx):
    t = tiled(gpu_ctx, 3)
    r, b, lim = t.r, t.b, R.LIMITS_OF[3]
    out = dict(phi=t.out("traj"), grad_coeff=t.out("coeff"), grad_times=t.out("seg"), peak=t.out("traj", 2))
    gpu_ctx.limit_penalty_device(r, t.n, 0, t.d_so, t.d_T, t.coeff, status=t.status, penalty=out["phi"], grad_coeff=out["grad_coeff"],
                                 grad_times=out["grad_times"], peak=out["peak"], **lim)
    gpu_ctx.synchronize()
    kinds = dict(phi="traj", grad_coeff="coeff", grad_times="seg", peak="traj")
    got = {k: t.copies_equal_the_base(v, kinds[k], k) for k, v in out.items()}
    for k in got:
        t.unsolved_is_zero(got[k], kinds[k], k)
    ref = L.penalty(r, b["so"], b["T_bad"], t.coeff0.cpu().numpy(), status=t.status0.cpu().numpy(), solved_value=U.UAVQP_SOLVED, **lim)
    assert np.count_nonzero(ref["phi"] > 0) >= 8 and np.count_nonzero(ref["phi"][t.ok] == 0) >= 8
    worst = worst_errors(b["so"], r, got, ref, tuple(kinds))
    print(f"limit penalty, {t.n} trajectories: copies bytes equal; base against the longdouble reference: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= PARITY, f"{k}: {v:.3e}"


def clearance_reference(t, ref_dist, params):
    b = t.b
    ref = E.penalty(t.r, b["so"], b["T_bad"], t.coeff0.cpu().numpy(), ref_dist, S.ORIGIN, S.MRES, S.MMAX, status=t.status0.cpu().numpy(),
                    solved_value=U.UAVQP_SOLVED, **params)
    assert np.count_nonzero(ref["phi"] > 0) >= 8 and np.count_nonzero(ref["phi"][t.ok] == 0) >= 8 and np.count_nonzero(ref["outside"] > 0) >= 1
    assert ref["margin"] >= 1e-6 and ref["gap"] >= 1e-9, (float(ref["margin"]), float(ref["gap"]))
    return ref


def test_clearance_penalty_past_one_grid(gpu_ctx, scene):
    m, ref_dist = scene
    t = tiled(gpu_ctx, 3)
    out = dict(phi=t.out("traj"), grad_coeff=t.out("coeff"), grad_times=t.out("seg"), min_dist=t.out("traj"), outside=t.out("traj", dtype=dev()[0].int32))
    gpu_ctx.clearance_penalty_device(t.r, t.n, 0, t.d_so, t.d_T, t.coeff, m, status=t.status, penalty=out["phi"], grad_coeff=out["grad_coeff"],
                                     grad_times=out["grad_times"], min_dist=out["min_dist"], outside=out["outside"], **S.PARAMS)
    gpu_ctx.synchronize()
    kinds = dict(phi="traj", grad_coeff="coeff", grad_times="seg", min_dist="traj", outside="traj")
    got = {k: t.copies_equal_the_base(v, kinds[k], k) for k, v in out.items()}
    for k in ("phi", "grad_coeff", "grad_times", "outside"):
        t.unsolved_is_zero(got[k], kinds[k], k)
    assert got["min_dist"][one_grid() + 5] == S.MMAX
    ref = clearance_reference(t, ref_dist, S.PARAMS)
    assert np.array_equal(got["outside"][:NB].astype(np.int64), ref["outside"])
    worst = worst_errors(t.b["so"], t.r, got, ref, ("phi", "grad_coeff", "grad_times", "min_dist"))
    print(f"clearance penalty, {t.n} trajectories: copies bytes equal; base against the longdouble reference: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= PARITY, f"{k}: {v:.3e}"


def test_flight_penalty_past_one_grid(gpu_ctx, scene):
    """r = 4 (the other entries: r = 3)"""
    torch, _ = dev()
    m, ref_dist = scene
    t = tiled(gpu_ctx, 4)
    r, b, lim_p = t.r, t.b, R.LIMITS_OF[4]
    out = dict(phi=t.out("traj"), grad_coeff=t.out("coeff"), grad_times=t.out("seg"), peak=t.out("traj", 2), min_dist=t.out("traj"),
               outside=t.out("traj", dtype=torch.int32))
    gpu_ctx.flight_penalty_device(r, t.n, 0, t.d_so, t.d_T, t.coeff, m, status=t.status, penalty=out["phi"], grad_coeff=out["grad_coeff"],
                                  grad_times=out["grad_times"], peak=out["peak"], min_dist=out["min_dist"], outside=out["outside"], limits=lim_p,
                                  clearance=S.PARAMS)
    gpu_ctx.synchronize()
    kinds = dict(phi="traj", grad_coeff="coeff", grad_times="seg", peak="traj", min_dist="traj", outside="traj")
    got = {k: t.copies_equal_the_base(v, kinds[k], k) for k, v in out.items()}
    for k in ("phi", "grad_coeff", "grad_times", "peak", "outside"):
        t.unsolved_is_zero(got[k], kinds[k], k)
    assert got["min_dist"][one_grid() + 5] == S.MMAX
    clr = clearance_reference(t, ref_dist, S.PARAMS)
    lim = L.penalty(r, b["so"], b["T_bad"], t.coeff0.cpu().numpy(), status=t.status0.cpu().numpy(), solved_value=U.UAVQP_SOLVED, **lim_p)
    assert np.count_nonzero(lim["phi"] > 0) >= 8
    ref = dict(phi=lim["phi"] + clr["phi"], grad_coeff=lim["grad_coeff"] + clr["grad_coeff"], grad_times=lim["grad_times"] + clr["grad_times"],
               peak=lim["peak"], min_dist=clr["min_dist"])
    assert np.array_equal(got["outside"][:NB].astype(np.int64), clr["outside"])
    worst = worst_errors(b["so"], r, got, ref, ("phi", "grad_coeff", "grad_times", "peak", "min_dist"))
    print(f"flight penalty r = 4, {t.n} trajectories: copies bytes equal; base against the longdouble references: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= PARITY, f"{k}: {v:.3e}"


def test_cost_waypoint_gradient_past_one_grid(gpu_ctx, oracle):
    """against 2 (P c)' dc/dp in longdouble on the oracle's coefficients, 1e-9 of the largest component (tests/test_gpu_waypoint_opt.py)"""
    t = tiled(gpu_ctx, 3)
    r, b = t.r, t.b
    grad = t.out("row", 3)
    gpu_ctx.cost_waypoint_gradient_device(r, t.n, 0, t.d_so, t.coeff, grad, status=t.status)
    gpu_ctx.synchronize()
    g = t.copies_equal_the_base(grad, "row", "grad")
    t.unsolved_is_zero(g, "row", "grad")
    worst = 0.0
    for k in np.flatnonzero(t.ok):
        s0, s1 = int(b["so"][k]), int(b["so"][k + 1])
        M, rows, T = s1 - s0, slice(s0 + k, s1 + k + 1), b["T"][s0:s1]
        P, _ = oracle.assemble(r, T)
        z = np.zeros(r - 1)
        Smat = np.column_stack([oracle.solve_exact(r, np.eye(M + 1)[j], z, z, T) for j in range(M + 1)]).astype(LD)
        want = np.zeros((M + 1, 3), dtype=LD)
        for ax in range(3):
            c_ref = oracle.solve_exact(r, b["wp"][rows, ax], b["bc"][k, 0, :, ax], b["bc"][k, 1, :, ax], T)
            want[:, ax] = 2.0 * (P.astype(LD) @ c_ref.astype(LD)) @ Smat
        worst = max(worst, float(np.max(np.abs(g[rows] - want)) / np.max(np.abs(want))))
    print(f"cost / waypoint gradient, {t.n} trajectories: copies bytes equal; |device - longdouble reference| / max component {worst:.3e}")
    assert worst <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- query, rasteriser
def test_query_past_one_grid(gpu_ctx, scene):
    torch, _ = dev()
    m, ref_dist = scene
    base = S.query_points()
    nb = base.shape[0]
    n = 256 * 32 * cus() + 77
    idx = up(np.arange(n, dtype=np.int64) % nb)
    d_pts = up(base)[idx]
    torch.cuda.synchronize()
    dist, grad, inside = m.query(d_pts)
    gpu_ctx.synchronize()
    for x, what in ((dist, "dist"), (grad, "grad"), (inside, "inside")):
        assert torch.equal(bits(x), bits(x)[idx]), f"{what}: a copy differs from its base point"
    want = E.query(ref_dist, S.ORIGIN, S.MRES, base)
    assert want["margin"].min() >= 1e-6
    dist, grad, inside = dist[:nb].cpu().numpy(), grad[:nb].cpu().numpy(), inside[:nb].cpu().numpy()
    assert np.array_equal(inside, want["inside"])
    scale = np.maximum(want["scale"], LD(S.MRES))
    e_d = float(np.max(np.abs(dist.astype(LD) - want["dist"]) / scale))
    e_g = float(np.max(np.abs(grad.astype(LD) - want["grad"]) * LD(S.MRES) / scale[:, None]))
    print(f"query, {n} points: copies bytes equal; dist {e_d:.3e}, grad * res {e_g:.3e} of max(|corner values|, res)")
    assert e_d <= 1e-13 and e_g <= 1e-13


def test_rasteriser_past_one_grid(gpu_ctx):
    """copies of the 200-point cloud, inflation (2, 2): 125 lanes per point.  Copy k is shifted by the whole voxels (k % 5 - 2,
    k / 5 % 5 - 2, k / 25 % 3 - 1); four copies -- the first, two in between and the last, whose lanes all lie in the stride round -- stay
    near the map, each pushed towards another face, and the others move 64 voxels out in x: 20 000 points in the map would fill all of
    it, and a lane that is skipped or mapped to the wrong point would change nothing."""
    base = S.raster_cloud()
    nb, cap = base.shape[0], 256 * 32 * cus()
    n_pts = max(20000, -(-(cap // 125 + 1 + nb) // nb) * nb)
    copies = n_pts // nb
    assert n_pts % nb == 0 and (n_pts - nb) * 125 >= cap
    k = np.arange(n_pts) // nb
    shift = np.column_stack([k % 5 - 2, k // 5 % 5 - 2, k // 25 % 3 - 1]).astype(np.float64)
    shift[:, 0] += 64.0
    for copy, near in ((0, (0, 0, 0)), (copies // 3, (0, 0, 12)), (2 * copies // 3, (0, 20, 0)), (copies - 1, (-25, 0, 0))):
        shift[k == copy] += np.array(near, dtype=np.float64) - np.array([64.0, 0.0, 0.0])
    cloud = base[np.arange(n_pts) % nb] + shift * S.MRES
    want, margin = E.rasterize(S.DIMS, S.ORIGIN, S.MRES, cloud, 2, 2)
    assert margin >= 1e-6, f"a point sits on a voxel face (margin {float(margin):.2e})"
    fill = np.count_nonzero(want) / want.size
    assert 0.2 < fill < 0.95
    without_last, _ = E.rasterize(S.DIMS, S.ORIGIN, S.MRES, cloud[:n_pts - nb], 2, 2)
    assert np.count_nonzero(want != without_last) >= 100, "the stride round would not be missed"
    with EsdfMap(gpu_ctx, S.DIMS, S.ORIGIN, S.MRES) as m:
        m.set_cloud(cloud, inflate_xy=2, inflate_z=2)
        got = m.read(sq_pos=False, sq_neg=False, dist=False)["occ"]
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} bytes differ"
    print(f"rasteriser, {n_pts} points x 125 offsets: bytes equal; {np.count_nonzero(want)} of {want.size} voxels occupied, "
          f"{np.count_nonzero(want != without_last)} of them by the stride round alone")


# ---------------------------------------------------------------------------------------------------------------- optimisers
ITERS = 6
SPLIT_KEYS = dict(T="seg", wp="row", coeff="coeff", status="traj", obj="traj", acc="traj", peak="traj", md="traj", outside="traj")


class Whole(Tiled):
    """the tiled batch as an optimiser's input: copy k of a trajectory starts from durations scaled by 1 + 0.02 (k % 11 - 5), so that
    accept / reject differs between the copies"""

    def __init__(self, ctx, r):
        super().__init__(ctx, r, one_grid() + 24)
        self.cut = 4 * 32 * cus() // 512 * 512
        assert self.cut >= 2048 and self.n - self.cut >= 2048, "the parts would not take the dealing by segment count of the whole"
        assert self.cut <= one_grid() and self.n - self.cut <= one_grid()
        factor = 1.0 + 0.02 * ((np.arange(self.n) // NB) % 11 - 5)
        self.d_T = self.d_T * up(np.repeat(factor, self.Ms))
        self.T_start, self.wp_start = self.d_T.cpu().numpy(), self.d_wp.cpu().numpy()

    def part(self, lo, hi):
        """-> (n, total, seg_offsets, waypoints, times, bc) of trajectories lo .. hi in allocations of their own"""
        so = self.so
        s0, s1 = int(so[lo]), int(so[hi])
        return (hi - lo, s1 - s0, up((so[lo:hi + 1] - s0).astype(np.int32)), self.d_wp[s0 + lo:s1 + hi].clone(), self.d_T[s0:s1].clone(),
                self.d_bc[lo:hi].clone())

    def run(self, entry, esdf, lo, hi):
        torch, d = dev()
        n, total, d_so, d_wp, d_T, d_bc = self.part(lo, hi)
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=d)
        o = dict(coeff=z(self.nc3 * total), status=z(n, dtype=torch.int32), obj=z(n, 2), acc=z(n, dtype=torch.int32), peak=z(n, 2), md=z(n),
                 outside=z(n, dtype=torch.int32))
        head = (self.r, n, 0, 3, total, d_so, d_wp, d_T, d_bc)
        lim, clr = R.LIMITS_OF[self.r], R.CLEARANCE
        torch.cuda.synchronize()
        if entry == "time":
            self.ctx.time_optimize_device(*head, o["coeff"], o["status"], o["obj"], o["acc"], max_iters=ITERS)
            keys = ("T", "coeff", "status", "obj", "acc")
        elif entry == "time_limits":
            self.ctx.time_optimize_limits_device(*head, o["coeff"], o["status"], o["obj"], o["acc"], peak_out=o["peak"], limits=lim, max_iters=ITERS)
            keys = ("T", "coeff", "status", "obj", "acc", "peak")
        elif entry == "waypoint":
            self.ctx.waypoint_optimize_device(*head, esdf, o["coeff"], o["status"], o["obj"], o["acc"], o["md"], o["outside"], clearance=clr,
                                              max_iters=ITERS, max_move=1.0)
            keys = ("wp", "coeff", "status", "obj", "acc", "md", "outside")
        else:
            self.ctx.spacetime_optimize_device(*head, esdf, o["coeff"], o["status"], o["obj"], o["acc"], o["peak"], o["md"], o["outside"], limits=lim,
                                               clearance=clr, max_iters=ITERS, max_move=1.0)
            keys = ("wp", "T", "coeff", "status", "obj", "acc", "peak", "md", "outside")
        self.ctx.synchronize()
        o["T"], o["wp"] = d_T, d_wp
        return {k: o[k] for k in keys}


_whole = {}


@pytest.mark.parametrize("entry", ["time", "time_limits", "waypoint", "spacetime"])
def test_optimiser_past_one_grid_equals_separate_calls(gpu_ctx, scene, entry):
    """per-trajectory state of the step kernels (step size, best objective, accept / reject) across launches, indexed by trajectory:
    one call past one grid gives the bytes of two calls that fit one grid each"""
    torch, _ = dev()
    m, _ = scene
    if 3 not in _whole:
        _whole[3] = Whole(gpu_ctx, 3)
    w = _whole[3]
    whole = w.run(entry, m, 0, w.n)
    so, cut, n = w.so, w.cut, w.n
    for lo, hi in ((0, cut), (cut, n)):
        part = w.run(entry, m, lo, hi)
        s0, s1 = int(so[lo]), int(so[hi])
        span = dict(traj=(lo, hi), seg=(s0, s1), row=(s0 + lo, s1 + hi), coeff=(w.nc3 * s0, w.nc3 * s1))
        for k, v in part.items():
            a, b = span[SPLIT_KEYS[k]]
            assert torch.equal(bits(whole[k][a:b].contiguous()), bits(v)), f"{entry}: {k} of trajectories {lo} .. {hi} differs between one call and two"
    # the stride round did something: the invalid trajectory is refused, the others moved, and not every trial was accepted
    tail = np.arange(one_grid(), n)
    st, acc = whole["status"].cpu().numpy(), whole["acc"].cpu().numpy()
    bad = one_grid() + 5
    assert st[bad] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st[tail], 5) == U.UAVQP_SOLVED) and acc[bad] == 0
    assert np.all(np.isnan(whole["obj"].cpu().numpy()[bad]))
    moved = np.zeros(n, dtype=bool)
    if "T" in whole:
        moved |= np.add.reduceat(whole["T"].cpu().numpy() != w.T_start, so[:-1]) > 0
    if "wp" in whole:
        moved |= np.add.reduceat(np.any(whole["wp"].cpu().numpy() != w.wp_start, axis=1), so[:-1] + np.arange(n)) > 0
    assert not moved[bad]
    valid = np.delete(tail, 5)
    rejected = np.count_nonzero((acc[valid] < ITERS) & moved[valid])
    print(f"{entry}: {n} trajectories in one call = {cut} + {n - cut} in two, bytes equal; stride round: {np.count_nonzero(moved[tail])} of {tail.size} "
          f"moved, accepted trials {acc[valid].min()} .. {acc[valid].max()} of {ITERS}, {rejected} moved and were rejected at least once")
    assert np.count_nonzero(moved[tail]) * 20 >= tail.size
    assert rejected >= 1 and np.count_nonzero(acc[valid] > 0) >= 1
    # the copies differ in their start, and so in their course
    first = np.flatnonzero(w.src == int(w.src[valid[0]]))
    assert len({int(a) for a in acc[first]}) > 1 or len({x.tobytes() for x in whole["obj"].cpu().numpy()[first]}) > 10
