"""The batched equality-constrained solve as a differentiable torch operation.

    coeff = solve_batch(ctx, r, waypoints, times, bc, uniform_segments=8)
    loss(coeff).backward()          # -> times.grad, waypoints.grad, bc.grad

forward = uavqp_solve_batch_device, backward = uavqp_solve_backward_device (include/uavqp.h), both enqueued on torch's current stream.
The gradients are the part THROUGH the minimiser; a loss that also depends on `times` explicitly (e.g. through sampling times that scale
with the durations) gets that part from torch's own graph, as for any other operation.  Inputs: contiguous float64 tensors on the
ctx's device.  No CPU path: without libuavqp.so or a GPU the call raises.  torch is imported when the operation is first used.

    phi = limit_penalty(ctx, r, coeff, times, uniform_segments=8, v_max=3.0)      # [n_traj]
    phi.sum().backward()            # coeff.grad, times.grad (the explicit part); through solve_batch: the total gradient

forward = uavqp_limit_penalty_device, which also writes both gradients; backward scales them by the incoming gradient per trajectory.

    phi = clearance_penalty(ctx, r, coeff, times, esdf, uniform_segments=8, d_safe=0.6)   # [n_traj], esdf: an updated esdf.EsdfMap

the same for uavqp_clearance_penalty_device; behind solve_batch the gradients reach waypoints, times and bc through its backward pass.

    phi = attitude_penalty(ctx, r, coeff, times, uniform_segments=8, tilt_max=0.5)        # [n_traj]

the same for uavqp_attitude_penalty_device (specific thrust, tilt and body rate of the vehicle that flies the trajectory).
"""
from . import _lib

_Function = None


def _function():
    global _Function
    if _Function is not None:
        return _Function
    import torch

    class SolveBatch(torch.autograd.Function):
        @staticmethod
        def forward(fctx, waypoints, times, bc, ctx, r, seg_offsets, uniform_segments, max_segments, check_status):
            for name, t in (("waypoints", waypoints), ("times", times), ("bc", bc)):
                if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"solve_batch: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if waypoints.numel() != 3 * (total + n_traj) or bc.numel() != n_traj * 2 * (r - 1) * 3:
                raise ValueError("solve_batch: waypoints must hold sum(M_b + 1) xyz rows and bc [n_traj][2][r-1][3]")
            coeff = torch.zeros(3 * 2 * r * total, dtype=torch.float64, device=times.device)
            status = torch.zeros(n_traj, dtype=torch.int32, device=times.device)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.solve_batch_device(r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints.detach(), times.detach(), bc.detach(),
                                   coeff, status)
            if check_status and not bool((status == _lib.UAVQP_SOLVED).all()):   # (a read-back: only on request)
                bad = int((status != _lib.UAVQP_SOLVED).sum())
                raise _lib.UavqpError(f"solve_batch: {bad} of {n_traj} trajectories did not solve")
            fctx.save_for_backward(waypoints, times, bc, coeff, status)
            fctx.call = (ctx, r, n_traj, uniform_segments, max_segments, total, seg_offsets)
            fctx.mark_non_differentiable(status)
            return coeff, status

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_coeff, _grad_status):
            waypoints, times, bc, coeff, status = fctx.saved_tensors
            ctx, r, n_traj, uniform_segments, max_segments, total, seg_offsets = fctx.call
            need_w, need_t, need_b = fctx.needs_input_grad[:3]
            g = grad_coeff.contiguous()
            g_w = torch.empty_like(waypoints) if need_w else None
            g_t = torch.empty_like(times) if need_t else None
            g_b = torch.empty_like(bc) if need_b else None
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.solve_backward_device(r, n_traj, uniform_segments, max_segments, total, seg_offsets, waypoints, times, bc, coeff, g,
                                      grad_times=g_t, grad_waypoints=g_w, grad_bc=g_b, status=status)
            return g_w, g_t, g_b, None, None, None, None, None, None

    _Function = SolveBatch
    return _Function


_Penalty = None


def _penalty_function():
    global _Penalty
    if _Penalty is not None:
        return _Penalty
    import torch

    class LimitPenalty(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coeff, times, ctx, r, seg_offsets, uniform_segments, status, limits):
            for name, t in (("coeff", coeff), ("times", times)):
                if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"limit_penalty: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if coeff.numel() != 3 * 2 * r * total:
                raise ValueError("limit_penalty: coeff must hold 3 * 2r doubles per segment")
            phi = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            g_c = torch.empty_like(coeff)
            g_t = torch.empty_like(times)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.limit_penalty_device(r, n_traj, uniform_segments, seg_offsets, times.detach(), coeff.detach(), status=status, penalty=phi,
                                     grad_coeff=g_c, grad_times=g_t, **limits)
            if uniform_segments > 0:
                counts = torch.full((n_traj,), uniform_segments, dtype=torch.int64, device=times.device)
            else:
                counts = (seg_offsets[1:] - seg_offsets[:-1]).to(torch.int64)
            fctx.save_for_backward(g_c, g_t, counts)
            fctx.nc = 3 * 2 * r
            return phi

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_phi):
            g_c, g_t, counts = fctx.saved_tensors
            need_c, need_t = fctx.needs_input_grad[:2]
            per_seg = torch.repeat_interleave(grad_phi, counts)                 # [sum M]
            out_c = g_c * torch.repeat_interleave(grad_phi, counts * fctx.nc) if need_c else None
            out_t = g_t * per_seg if need_t else None
            return out_c, out_t, None, None, None, None, None, None

    _Penalty = LimitPenalty
    return _Penalty


_Attitude = None


def _attitude_function():
    global _Attitude
    if _Attitude is not None:
        return _Attitude
    import torch

    class AttitudePenalty(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coeff, times, ctx, r, seg_offsets, uniform_segments, status, params):
            for name, t in (("coeff", coeff), ("times", times)):
                if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"attitude_penalty: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if coeff.numel() != 3 * 2 * r * total:
                raise ValueError("attitude_penalty: coeff must hold 3 * 2r doubles per segment")
            phi = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            g_c = torch.empty_like(coeff)
            g_t = torch.empty_like(times)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.attitude_penalty_device(r, n_traj, uniform_segments, seg_offsets, times.detach(), coeff.detach(), status=status, penalty=phi,
                                        grad_coeff=g_c, grad_times=g_t, **params)
            if uniform_segments > 0:
                counts = torch.full((n_traj,), uniform_segments, dtype=torch.int64, device=times.device)
            else:
                counts = (seg_offsets[1:] - seg_offsets[:-1]).to(torch.int64)
            fctx.save_for_backward(g_c, g_t, counts)
            fctx.nc = 3 * 2 * r
            return phi

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_phi):
            g_c, g_t, counts = fctx.saved_tensors
            need_c, need_t = fctx.needs_input_grad[:2]
            out_c = g_c * torch.repeat_interleave(grad_phi, counts * fctx.nc) if need_c else None
            out_t = g_t * torch.repeat_interleave(grad_phi, counts) if need_t else None
            return out_c, out_t, None, None, None, None, None, None

    _Attitude = AttitudePenalty
    return _Attitude


_Clearance = None


def _clearance_function():
    global _Clearance
    if _Clearance is not None:
        return _Clearance
    import torch

    class ClearancePenalty(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coeff, times, ctx, r, esdf, seg_offsets, uniform_segments, status, params):
            for name, t in (("coeff", coeff), ("times", times)):
                if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"clearance_penalty: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if coeff.numel() != 3 * 2 * r * total:
                raise ValueError("clearance_penalty: coeff must hold 3 * 2r doubles per segment")
            phi = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            g_c = torch.empty_like(coeff)
            g_t = torch.empty_like(times)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.clearance_penalty_device(r, n_traj, uniform_segments, seg_offsets, times.detach(), coeff.detach(), esdf, status=status,
                                         penalty=phi, grad_coeff=g_c, grad_times=g_t, **params)
            if uniform_segments > 0:
                counts = torch.full((n_traj,), uniform_segments, dtype=torch.int64, device=times.device)
            else:
                counts = (seg_offsets[1:] - seg_offsets[:-1]).to(torch.int64)
            fctx.save_for_backward(g_c, g_t, counts)
            fctx.nc = 3 * 2 * r
            return phi

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_phi):
            g_c, g_t, counts = fctx.saved_tensors
            need_c, need_t = fctx.needs_input_grad[:2]
            out_c = g_c * torch.repeat_interleave(grad_phi, counts * fctx.nc) if need_c else None
            out_t = g_t * torch.repeat_interleave(grad_phi, counts) if need_t else None
            return out_c, out_t, None, None, None, None, None, None, None

    _Clearance = ClearancePenalty
    return _Clearance


_Flight = None


def _flight_function():
    global _Flight
    if _Flight is not None:
        return _Flight
    import torch

    class FlightPenalty(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coeff, times, ctx, r, esdf, seg_offsets, uniform_segments, status, limits, clearance):
            for name, t in (("coeff", coeff), ("times", times)):
                if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
                    raise ValueError(f"flight_penalty: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if coeff.numel() != 3 * 2 * r * total:
                raise ValueError("flight_penalty: coeff must hold 3 * 2r doubles per segment")
            phi = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            g_c = torch.empty_like(coeff)
            g_t = torch.empty_like(times)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.flight_penalty_device(r, n_traj, uniform_segments, seg_offsets, times.detach(), coeff.detach(), esdf, status=status,
                                      penalty=phi, grad_coeff=g_c, grad_times=g_t, limits=limits, clearance=clearance)
            if uniform_segments > 0:
                counts = torch.full((n_traj,), uniform_segments, dtype=torch.int64, device=times.device)
            else:
                counts = (seg_offsets[1:] - seg_offsets[:-1]).to(torch.int64)
            fctx.save_for_backward(g_c, g_t, counts)
            fctx.nc = 3 * 2 * r
            return phi

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_phi):
            g_c, g_t, counts = fctx.saved_tensors
            need_c, need_t = fctx.needs_input_grad[:2]
            out_c = g_c * torch.repeat_interleave(grad_phi, counts * fctx.nc) if need_c else None
            out_t = g_t * torch.repeat_interleave(grad_phi, counts) if need_t else None
            return out_c, out_t, None, None, None, None, None, None, None, None

    _Flight = FlightPenalty
    return _Flight


_Swarm = None


def _swarm_function():
    global _Swarm
    if _Swarm is not None:
        return _Swarm
    import torch

    class SwarmPenalty(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coeff, times, start, ctx, r, group_offsets, seg_offsets, uniform_segments, status, params):
            for name, t in (("coeff", coeff), ("times", times), ("start", start)):
                if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous()):
                    raise ValueError(f"swarm_penalty: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if coeff.numel() != 3 * 2 * r * total:
                raise ValueError("swarm_penalty: coeff must hold 3 * 2r doubles per segment")
            if start is not None and start.numel() != n_traj:
                raise ValueError("swarm_penalty: start must hold one departure time per trajectory")
            n_groups = 1 if group_offsets is None else group_offsets.numel() - 1
            phi = torch.empty(n_groups, dtype=torch.float64, device=times.device)
            g_c = torch.empty_like(coeff)
            g_t = torch.empty_like(times)
            g_s = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            ctx.swarm_penalty_device(r, n_traj, uniform_segments, seg_offsets, times.detach(), coeff.detach(), n_groups=n_groups,
                                     group_offsets=group_offsets, start=None if start is None else start.detach(), status=status,
                                     penalty=phi, grad_coeff=g_c, grad_times=g_t, grad_start=g_s, **params)
            if uniform_segments > 0:
                counts = torch.full((n_traj,), uniform_segments, dtype=torch.int64, device=times.device)
            else:
                counts = (seg_offsets[1:] - seg_offsets[:-1]).to(torch.int64)
            if group_offsets is None:
                sizes = torch.full((1,), n_traj, dtype=torch.int64, device=times.device)
            else:
                sizes = (group_offsets[1:] - group_offsets[:-1]).to(torch.int64)
            fctx.save_for_backward(g_c, g_t, g_s, counts, sizes)
            fctx.nc = 3 * 2 * r
            return phi

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_phi):
            g_c, g_t, g_s, counts, sizes = fctx.saved_tensors
            need_c, need_t, need_s = fctx.needs_input_grad[:3]
            per_traj = torch.repeat_interleave(grad_phi, sizes)                    # the swarm's weight on each of its vehicles
            out_c = g_c * torch.repeat_interleave(per_traj, counts * fctx.nc) if need_c else None
            out_t = g_t * torch.repeat_interleave(per_traj, counts) if need_t else None
            out_s = g_s * per_traj if need_s else None
            return out_c, out_t, out_s, None, None, None, None, None, None, None

    _Swarm = SwarmPenalty
    return _Swarm


_Moving = None


def _moving_function():
    global _Moving
    if _Moving is not None:
        return _Moving
    import torch

    class MovingPenalty(torch.autograd.Function):
        @staticmethod
        def forward(fctx, coeff, times, traj_start, ctx, r, obstacles, seg_offsets, uniform_segments, status, params):
            for name, t in (("coeff", coeff), ("times", times), ("traj_start", traj_start)):
                if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous()):
                    raise ValueError(f"moving_penalty: {name} must be a contiguous float64 tensor on the GPU")
            total = times.numel()
            n_traj = total // uniform_segments if uniform_segments > 0 else seg_offsets.numel() - 1
            if coeff.numel() != 3 * 2 * r * total:
                raise ValueError("moving_penalty: coeff must hold 3 * 2r doubles per segment")
            if traj_start is not None and traj_start.numel() != n_traj:
                raise ValueError("moving_penalty: traj_start must hold one departure time per trajectory")
            phi = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            g_c = torch.empty_like(coeff)
            g_t = torch.empty_like(times)
            g_s = torch.empty(n_traj, dtype=torch.float64, device=times.device)
            ctx.set_stream(torch.cuda.current_stream(times.device).cuda_stream)
            obs = dict(obstacles, traj_start=None if traj_start is None else traj_start.detach())
            ctx.moving_penalty_device(r, n_traj, uniform_segments, seg_offsets, times.detach(), coeff.detach(), obs, status=status, penalty=phi,
                                      grad_coeff=g_c, grad_times=g_t, grad_start=g_s, **params)
            if uniform_segments > 0:
                counts = torch.full((n_traj,), uniform_segments, dtype=torch.int64, device=times.device)
            else:
                counts = (seg_offsets[1:] - seg_offsets[:-1]).to(torch.int64)
            fctx.save_for_backward(g_c, g_t, g_s, counts)
            fctx.nc = 3 * 2 * r
            return phi

        @staticmethod
        @torch.autograd.function.once_differentiable   # the gradients come from a raw kernel: no second derivative through them
        def backward(fctx, grad_phi):
            g_c, g_t, g_s, counts = fctx.saved_tensors
            need_c, need_t, need_s = fctx.needs_input_grad[:3]
            out_c = g_c * torch.repeat_interleave(grad_phi, counts * fctx.nc) if need_c else None
            out_t = g_t * torch.repeat_interleave(grad_phi, counts) if need_t else None
            out_s = g_s * grad_phi if need_s else None
            return out_c, out_t, out_s, None, None, None, None, None, None, None

    _Moving = MovingPenalty
    return _Moving


def solve_batch(ctx, r, waypoints, times, bc, seg_offsets=None, uniform_segments=0, max_segments=0, check_status=False, return_status=False):
    """Differentiable uavqp_solve_batch_device.  ctx: a Context on the tensors' device.  waypoints [sum (M_b + 1)][3], times [sum M_b],
    bc [n_traj][2][r-1][3]; seg_offsets: int32 device tensor [n_traj + 1] (ragged; max_segments = the longest trajectory, read back from
    the offsets when 0) or None with uniform_segments > 0.  Returns coeff [sum_b 3 * M_b * 2r] (layout [axis][segment][2r] per
    trajectory), with return_status also the int32 status tensor.  A trajectory that does not solve carries zero gradient;
    check_status=True raises UavqpError instead (it costs a read-back)."""
    if uniform_segments <= 0:
        if seg_offsets is None:
            raise ValueError("solve_batch: ragged batches need seg_offsets")
        if max_segments <= 0:
            max_segments = max(int((seg_offsets[1:] - seg_offsets[:-1]).max()), 1)
    else:
        max_segments = uniform_segments
    coeff, status = _function().apply(waypoints, times, bc, ctx, int(r), seg_offsets, int(uniform_segments), int(max_segments), bool(check_status))
    return (coeff, status) if return_status else coeff


def limit_penalty(ctx, r, coeff, times, seg_offsets=None, uniform_segments=0, status=None, **limits):
    """Differentiable uavqp_limit_penalty_device: the velocity / acceleration limit penalty [n_traj] of coeff (layout of solve_batch's
    result) at the durations `times` [sum M_b].  limits: fields of uavqp_limit_params that differ from the defaults (v_max, a_max,
    weight_v, weight_a, samples_per_seg).  status: optional int32 status tensor of the solve (trajectories that are not SOLVED give zero).
    The gradient in `times` is the explicit part; with coeff = solve_batch(..., times, ...) torch adds the part through the solve, so
    limit_penalty(solve_batch(...), times).sum().backward() leaves the total gradient in times.grad."""
    if uniform_segments <= 0 and seg_offsets is None:
        raise ValueError("limit_penalty: ragged batches need seg_offsets")
    return _penalty_function().apply(coeff, times, ctx, int(r), seg_offsets, int(uniform_segments), status, dict(limits))


def attitude_penalty(ctx, r, coeff, times, seg_offsets=None, uniform_segments=0, status=None, **params):
    """Differentiable uavqp_attitude_penalty_device: the thrust / tilt / body-rate penalty [n_traj] of coeff (layout of solve_batch's
    result) at the durations `times` [sum M_b].  params: fields of uavqp_attitude_params that differ from the defaults (gravity, f_min,
    f_max, tilt_max, rate_max, weight_thrust, weight_tilt, weight_rate, samples_per_seg).  status: optional int32 status tensor of the
    solve.  The gradient in `times` is the explicit part; with coeff = solve_batch(..., times, ...) torch adds the part through the solve,
    and waypoints.grad / bc.grad come from the same backward pass."""
    if uniform_segments <= 0 and seg_offsets is None:
        raise ValueError("attitude_penalty: ragged batches need seg_offsets")
    from .traj_optimizer import Context
    Context._attitude_params(params)   # (an unknown field is refused before anything runs)
    return _attitude_function().apply(coeff, times, ctx, int(r), seg_offsets, int(uniform_segments), status, dict(params))


def clearance_penalty(ctx, r, coeff, times, esdf, seg_offsets=None, uniform_segments=0, status=None, **params):
    """Differentiable uavqp_clearance_penalty_device: the clearance penalty [n_traj] of coeff (layout of solve_batch's result) at the
    durations `times` [sum M_b] against the distance field `esdf` (an esdf.EsdfMap on ctx, updated).  params: fields of
    uavqp_clearance_params that differ from the defaults (samples_per_seg, d_safe, weight).  status: optional int32 status tensor of the
    solve.  The gradient in `times` is the explicit part; with coeff = solve_batch(..., times, ...) torch adds the part through the solve,
    and waypoints.grad / bc.grad come from the same backward pass."""
    if uniform_segments <= 0 and seg_offsets is None:
        raise ValueError("clearance_penalty: ragged batches need seg_offsets")
    return _clearance_function().apply(coeff, times, ctx, int(r), esdf, seg_offsets, int(uniform_segments), status, dict(params))


def swarm_penalty(ctx, r, coeff, times, group_offsets=None, start=None, seg_offsets=None, uniform_segments=0, status=None, **params):
    """Differentiable uavqp_swarm_penalty_device: the separation penalty [n_groups] between the vehicles of each swarm (trajectories
    group_offsets[g] .. group_offsets[g + 1], an int32 device tensor; None: the whole batch is one swarm) of coeff (layout of
    solve_batch's result) at the durations `times` [sum M_b] and the departure times `start` [n_traj] (None: all zero, not
    differentiated).  params: fields of uavqp_swarm_params that differ from the defaults (n_samples, clock_start, dt, d_safe, downwash,
    weight).  status: optional int32 status tensor of the solve.  Differentiable in coeff, times and start; an upstream weight per swarm
    scales that swarm's gradients.  The gradient in `times` is the explicit part; with coeff = solve_batch(..., times, ...) torch adds
    the part through the solve, and waypoints.grad / bc.grad come from the same backward pass."""
    if uniform_segments <= 0 and seg_offsets is None:
        raise ValueError("swarm_penalty: ragged batches need seg_offsets")
    from .traj_optimizer import Context
    Context._swarm_params(params)   # (an unknown field is refused before anything runs)
    return _swarm_function().apply(coeff, times, start, ctx, int(r), group_offsets, seg_offsets, int(uniform_segments), status, dict(params))


def moving_penalty(ctx, r, coeff, times, obstacles, traj_start=None, seg_offsets=None, uniform_segments=0, status=None, **params):
    """Differentiable uavqp_moving_penalty_device: the penalty [n_traj] of coeff (layout of solve_batch's result) at the durations `times`
    [sum M_b] and the departures `traj_start` [n_traj] (None: all zero, not differentiated) against the MOVING obstacle tracks
    `obstacles`: the dict Context.moving_penalty_device takes (n_obs, uniform_segments, n_sets and the device tensors seg_offsets, times,
    coeff, start, radius, set_offsets, traj_set), without traj_start.  params: fields of uavqp_moving_params that differ from the defaults
    (samples_per_seg, d_safe, downwash, weight).  status: optional int32 status tensor of the solve.  Differentiable in coeff, times and
    traj_start, not in the obstacles.  The gradient in `times` is the explicit part; with coeff = solve_batch(..., times, ...) torch adds
    the part through the solve, and waypoints.grad / bc.grad come from the same backward pass."""
    if uniform_segments <= 0 and seg_offsets is None:
        raise ValueError("moving_penalty: ragged batches need seg_offsets")
    if "traj_start" in obstacles:
        raise ValueError("moving_penalty: traj_start is an argument of its own")
    from .traj_optimizer import Context
    Context._moving_params(params)   # (an unknown field is refused before anything runs)
    Context._moving_obstacles(obstacles)
    return _moving_function().apply(coeff, times, traj_start, ctx, int(r), dict(obstacles), seg_offsets, int(uniform_segments), status,
                                    dict(params))


def flight_penalty(ctx, r, coeff, times, esdf, seg_offsets=None, uniform_segments=0, status=None, limits=None, clearance=None):
    """Differentiable uavqp_flight_penalty_device: limit penalty + clearance penalty [n_traj] of coeff (layout of solve_batch's result) at
    the durations `times` [sum M_b] against the distance field `esdf` (an esdf.EsdfMap on ctx, updated), in one launch.  limits / clearance:
    dicts of uavqp_limit_params / uavqp_clearance_params fields that differ from the defaults.  status: optional int32 status tensor of
    the solve.  The gradient in `times` is the explicit part; with coeff = solve_batch(..., times, ...) torch adds the part through the
    solve, and waypoints.grad / bc.grad come from the same backward pass."""
    if uniform_segments <= 0 and seg_offsets is None:
        raise ValueError("flight_penalty: ragged batches need seg_offsets")
    return _flight_function().apply(coeff, times, ctx, int(r), esdf, seg_offsets, int(uniform_segments), status, dict(limits or {}),
                                    dict(clearance or {}))
