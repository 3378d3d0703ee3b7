"""GPU: a replayed capture may run solves side by side when their buffers do not overlap (uavqp_capture_end rebuilds the captured
chain from what each launch touches: csrc/uavqp_capture.h).  Every case compares, BITWISE, every buffer after a replay with the same
calls made eagerly in the same order on fresh buffers -- on the first replay and on the second.  Which edges the analysis draws is
pinned by tests/test_capture_deps.py; here only results count."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (r, M, n): sixteen tile-4 waves; a shifted partial tile; min-jerk with an odd segment count
SHAPES = [(4, 8, 64), (4, 8, 37), (3, 5, 64)]
COEFF_FILL, STATUS_FILL = -7.25, -99


@pytest.fixture(autouse=True)
def lanes_for_short_captures(monkeypatch):
    """By default a lane is used only where a stage has 16 launches for it (a shorter one replays faster as the chain it was captured as).
    The captures here have 2 to 13 launches: UAVQP_CAPTURE_LANE_NODES=1 (read when a capture ends) puts them on lanes all the same."""
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")


def _torch():
    import torch
    return torch


def _inputs(r, M, n, seed, bad=None):
    """Host inputs of one uniform solve; bad = (trajectory, segment): a non-positive duration there."""
    from uav_motion_planning_amd import workloads as W
    b = W.uniform_batch(2, n, M, r, time_mode="distance", seed=seed)
    T = np.array(b["times"], dtype=np.float64)
    if bad is not None:
        T[bad[0], bad[1]] = -0.5
    return (np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1), T.reshape(-1),
            np.ascontiguousarray(b["bc"], dtype=np.float64).reshape(-1))


def _bits(t):
    torch = _torch()
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else t.dtype).cpu().numpy().copy()


def _check(ctx, make, enqueue, replays=2):
    """make() -> dict of fresh device tensors (the same values every time); enqueue(ctx, bufs) makes the calls.  Eager first (it also sizes
    the workspaces), then the capture on a second set of buffers, re-initialised in place before each replay."""
    torch = _torch()
    eager = make()
    torch.cuda.synchronize()
    enqueue(ctx, eager)
    ctx.synchronize()
    want = {k: _bits(v) for k, v in eager.items()}
    bufs = make()
    torch.cuda.synchronize()
    ctx.capture_begin()
    try:
        enqueue(ctx, bufs)
    finally:
        graph = ctx.capture_end()
    try:
        for replay in range(replays):
            if replay:
                for k, v in make().items():
                    bufs[k].copy_(v)
                torch.cuda.synchronize()
            ctx.graph_launch(graph)
            ctx.synchronize()
            for k in want:
                got = _bits(bufs[k])
                assert np.array_equal(got, want[k]), f"replay {replay + 1}: buffer {k!r} differs from eager order in {int((got != want[k]).sum())} words"
    finally:
        ctx.graph_destroy(graph)
    return eager


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _fill(count, kind):
    """An output array nothing has written yet: kind "d" = doubles, "i" = int32 statuses."""
    torch = _torch()
    if kind == "i":
        return torch.full((int(count),), STATUS_FILL, dtype=torch.int32, device="cuda:0")
    return torch.full((int(count),), COEFF_FILL, dtype=torch.float64, device="cuda:0")


def _n_coeff(r, M, n):
    return 3 * 2 * r * n * M


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_twelve_solves_over_three_buffer_sets_sharing_one_status(gpu_ctx, r, M, n):
    def make():
        bufs = {"st": _fill(n, "i")}
        for s in range(3):
            wp, T, bc = _inputs(r, M, n, seed=100 + s, bad=(5, 1) if s == 1 else None)
            bufs.update({f"wp{s}": _dev(wp), f"T{s}": _dev(T), f"bc{s}": _dev(bc), f"out{s}": _fill(_n_coeff(r, M, n), "d")})
        return bufs

    def enqueue(ctx, b):
        for i in range(12):
            s = i % 3
            ctx.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], b["st"])

    eager = _check(gpu_ctx, make, enqueue)
    st = eager["st"].cpu().numpy()
    import uav_motion_planning_amd as U
    assert np.all(st == U.UAVQP_SOLVED)                       # the last writer is set 2 (clean); set 1's invalid trajectory left no trace
    assert not np.any(_bits(eager["out0"]) == np.float64(COEFF_FILL).view(np.int64))


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_read_after_write_durations_from_coefficients(gpu_ctx, r, M, n):
    """Solve B takes its durations from a 16-byte aligned slice of solve A's coefficients (many are not positive: invalid input)."""
    def make():
        wa, Ta, bca = _inputs(r, M, n, seed=7)
        wb, _, bcb = _inputs(r, M, n, seed=8)
        return {"wa": _dev(wa), "Ta": _dev(Ta), "bca": _dev(bca), "outa": _fill(_n_coeff(r, M, n), "d"), "sta": _fill(n, "i"),
                "wb": _dev(wb), "bcb": _dev(bcb), "outb": _fill(_n_coeff(r, M, n), "d"), "stb": _fill(n, "i")}

    def enqueue(ctx, b):
        ctx.solve_batch_device(r, n, M, M, None, b["wa"], b["Ta"], b["bca"], b["outa"], b["sta"])
        ctx.solve_batch_device(r, n, M, M, None, b["wb"], b["outa"][2:2 + n * M], b["bcb"], b["outb"], b["stb"])

    eager = _check(gpu_ctx, make, enqueue)
    import uav_motion_planning_amd as U
    stb = eager["stb"].cpu().numpy()
    assert np.any(stb == U.UAVQP_INVALID_INPUT) and not np.any(stb == STATUS_FILL)


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_write_after_read_coefficients_over_boundary_values(gpu_ctx, r, M, n):
    """Solve B writes its coefficients over the array solve A reads its boundary values from."""
    n_bc = n * 2 * (r - 1) * 3

    def make():
        wa, Ta, bca = _inputs(r, M, n, seed=17)
        wb, Tb, bcb = _inputs(r, M, n, seed=18)
        shared = _fill(_n_coeff(r, M, n), "d")
        shared[4:4 + n_bc] = _dev(bca)
        return {"wa": _dev(wa), "Ta": _dev(Ta), "shared": shared, "outa": _fill(_n_coeff(r, M, n), "d"), "sta": _fill(n, "i"),
                "wb": _dev(wb), "Tb": _dev(Tb), "bcb": _dev(bcb), "stb": _fill(n, "i")}

    def enqueue(ctx, b):
        ctx.solve_batch_device(r, n, M, M, None, b["wa"], b["Ta"], b["shared"][4:4 + n_bc], b["outa"], b["sta"])
        ctx.solve_batch_device(r, n, M, M, None, b["wb"], b["Tb"], b["bcb"], b["shared"], b["stb"])

    _check(gpu_ctx, make, enqueue)


@pytest.mark.parametrize("r,M,n", SHAPES)
@pytest.mark.parametrize("order,b_offset", [("AB", 0), ("BA", 0), ("AB", 16), ("BA", 16)])
def test_status_of_two_solves_in_one_array(gpu_ctx, r, M, n, order, b_offset):
    """A has a non-positive duration in trajectory 3, B is clean; both report into one status array (B's view shifted by b_offset)."""
    import uav_motion_planning_amd as U

    def make():
        wa, Ta, bca = _inputs(r, M, n, seed=27, bad=(3, 2))
        wb, Tb, bcb = _inputs(r, M, n, seed=28)
        return {"wa": _dev(wa), "Ta": _dev(Ta), "bca": _dev(bca), "outa": _fill(_n_coeff(r, M, n), "d"),
                "wb": _dev(wb), "Tb": _dev(Tb), "bcb": _dev(bcb), "outb": _fill(_n_coeff(r, M, n), "d"), "st": _fill(n + 16, "i")}

    def enqueue(ctx, b):
        for which in order:
            if which == "A":
                ctx.solve_batch_device(r, n, M, M, None, b["wa"], b["Ta"], b["bca"], b["outa"], b["st"][:n])
            else:
                ctx.solve_batch_device(r, n, M, M, None, b["wb"], b["Tb"], b["bcb"], b["outb"], b["st"][b_offset:b_offset + n])

    st = _check(gpu_ctx, make, enqueue)["st"].cpu().numpy()
    if b_offset == 0:
        want = np.full(n + 16, STATUS_FILL)
        want[:n] = U.UAVQP_SOLVED
        if order == "BA":
            want[3] = U.UAVQP_INVALID_INPUT
        assert np.array_equal(st, want)
    else:
        assert st[3] == U.UAVQP_INVALID_INPUT and np.all(st[16:] == U.UAVQP_SOLVED)    # B's view starts behind trajectory 3


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_evaluation_captured_between_two_solves(gpu_ctx, r, M, n):
    """A launch of another entry point in the capture: the graph stays the chain it was captured as."""
    ns = 9

    def make():
        wa, Ta, bca = _inputs(r, M, n, seed=37)
        wb, Tb, bcb = _inputs(r, M, n, seed=38)
        return {"wa": _dev(wa), "Ta": _dev(Ta), "bca": _dev(bca), "outa": _fill(_n_coeff(r, M, n), "d"), "sta": _fill(n, "i"),
                "wb": _dev(wb), "Tb": _dev(Tb), "bcb": _dev(bcb), "outb": _fill(_n_coeff(r, M, n), "d"), "stb": _fill(n, "i"),
                "ev": _fill(n * ns * 9, "d")}

    def enqueue(ctx, b):
        ctx.solve_batch_device(r, n, M, M, None, b["wa"], b["Ta"], b["bca"], b["outa"], b["sta"])
        ctx.eval_batch_device(r, n, M, None, b["Ta"], b["outa"], ns, 0.0, 0.17, 7, b["ev"])
        ctx.solve_batch_device(r, n, M, M, None, b["wb"], b["Tb"], b["bcb"], b["outb"], b["stb"])

    eager = _check(gpu_ctx, make, enqueue)
    assert not np.any(_bits(eager["ev"]) == np.float64(COEFF_FILL).view(np.int64))


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_ragged_solve_among_uniform_ones(gpu_ctx, r, M, n):
    from uav_motion_planning_amd import workloads as W
    rag = W.ragged_batch(4, n, r, m_lo=2, m_hi=7, seed=47)
    tot = int(rag["seg_offsets"][-1])

    def make():
        bufs = {"st": _fill(n, "i"), "so": _dev(rag["seg_offsets"]), "wr": _dev(rag["waypoints"].reshape(-1)), "Tr": _dev(rag["times"]),
                "bcr": _dev(rag["bc"].reshape(-1)), "outr": _fill(3 * 2 * r * tot, "d"), "str": _fill(n, "i")}
        for s in range(4):
            wp, T, bc = _inputs(r, M, n, seed=50 + s)
            bufs.update({f"wp{s}": _dev(wp), f"T{s}": _dev(T), f"bc{s}": _dev(bc), f"out{s}": _fill(_n_coeff(r, M, n), "d")})
        return bufs

    def enqueue(ctx, b):
        for s in range(4):
            if s == 2:
                ctx.solve_batch_device(r, n, 0, 7, b["so"], b["wr"], b["Tr"], b["bcr"], b["outr"], b["str"])
            ctx.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], b["st"])

    import uav_motion_planning_amd as U
    eager = _check(gpu_ctx, make, enqueue)
    assert np.all(eager["str"].cpu().numpy() == U.UAVQP_SOLVED) and np.all(eager["st"].cpu().numpy() == U.UAVQP_SOLVED)


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_one_lane_replays_the_captured_chain(r, M, n):
    """UAVQP_CAPTURE_LANES=1 (read when a capture ends): same outputs."""
    import uav_motion_planning_amd as U
    before = os.environ.get("UAVQP_CAPTURE_LANES")
    os.environ["UAVQP_CAPTURE_LANES"] = "1"
    try:
        with U.Context(0) as ctx:
            def make():
                bufs = {"st": _fill(n, "i")}
                for s in range(3):
                    wp, T, bc = _inputs(r, M, n, seed=60 + s, bad=(3, 0) if s == 2 else None)
                    bufs.update({f"wp{s}": _dev(wp), f"T{s}": _dev(T), f"bc{s}": _dev(bc), f"out{s}": _fill(_n_coeff(r, M, n), "d")})
                return bufs

            def enqueue(c, b):
                for i in range(6):
                    s = i % 3
                    c.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], b["st"])

            st = _check(ctx, make, enqueue)["st"].cpu().numpy()
            assert st[3] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st, 3) == U.UAVQP_SOLVED)
    finally:
        if before is None:
            del os.environ["UAVQP_CAPTURE_LANES"]
        else:
            os.environ["UAVQP_CAPTURE_LANES"] = before
