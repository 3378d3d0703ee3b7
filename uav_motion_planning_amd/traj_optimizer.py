"""Host-side mirror of the reference optimiser interface over the C ABI (include/uavqp.h).

  * MinimumControl  -- same method names / argument meaning / error behaviour as
    traj_optimization::MinimumControl (reference minimum_control.h:10-48, minimum_control.cpp:127-202):
    solve(pos_1d, bound_vel, bound_acc, time_vec) -> bool, getCoef1d(), reset().
  * TrajOptimizer   -- the batch facade named by BASELINE.json's north_star
    (setWaypoints / setTimeAllocation / solve / getPolyCoeff); no reference counterpart.
  * Context         -- thin RAII wrapper of uavqp_ctx for callers that already hold device buffers.

torch is used only for device memory and streams.  No CPU fallback: without libuavqp.so or without a
GPU every solve raises / returns False exactly as the reference does on solver failure.
"""
import ctypes
import functools

import numpy as np

from . import _lib


def _ptr(x):
    """Raw address of a numpy array / torch tensor; None and a raw integer address pass through."""
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if x is None or isinstance(x, int):
        return x
    return x.data_ptr()  # torch tensor


def _unknown_field(c_name, k):
    return ValueError(f"unknown uavqp_{c_name} field {k!r}")


def _batch_shape(seg_offsets, times, uniform_segments):
    """(seg_offsets as int32 or None, n_traj, total segments, longest trajectory) of a host batch."""
    if uniform_segments > 0:
        n_traj = times.size // uniform_segments
        return None, n_traj, n_traj * uniform_segments, uniform_segments
    so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
    n_traj = so.size - 1
    return so, n_traj, (int(so[-1]) if n_traj > 0 else 0), (int(np.max(np.diff(so))) if n_traj > 0 else 1)


class Context:
    """Owns one uavqp_ctx (one per host thread / device, as MinimumControl owns one OsqpEigen::Solver)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().uavqp_create(ctypes.byref(self._h), int(device)), "uavqp_create")
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().uavqp_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream_handle):
        """hip_stream_handle: integer hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or None."""
        _lib.check(_lib.lib().uavqp_set_stream(self._h, ctypes.c_void_p(hip_stream_handle or 0)), "uavqp_set_stream")

    def set_variant(self, variant):
        _lib.check(_lib.lib().uavqp_set_variant(self._h, int(variant)), "uavqp_set_variant")

    def synchronize(self):
        _lib.check(_lib.lib().uavqp_synchronize(self._h), "uavqp_synchronize")

    def get_settings(self):
        """Current uavqp_settings of this ctx (a _lib.Settings ctypes struct)."""
        st = _lib.Settings()
        _lib.check(_lib.lib().uavqp_get_settings(self._h, ctypes.byref(st)), "uavqp_get_settings")
        return st

    def set_settings(self, **fields):
        """Update fields of the ctx's uavqp_settings (reference: minimum_control.cpp:160-162 sets warm_start,
        eps_prim_inf, max_iter on its OsqpEigen solver), e.g. set_settings(max_iter=1000, ragged_window_sort=0)."""
        st = self.get_settings()
        for k, v in fields.items():
            if not hasattr(st, k):
                raise AttributeError(f"uavqp_settings has no field {k!r}")
            setattr(st, k, v)
        _lib.check(_lib.lib().uavqp_set_settings(self._h, ctypes.byref(st)), "uavqp_set_settings")

    def eval_batch_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, n_samples, t0, dt, what, out):
        """Batched PolyTraj::evaluatePos/Vel/Acc on the grid t0 + s*dt (device buffers, asynchronous)."""
        rc = _lib.lib().uavqp_eval_batch_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                n_samples, float(t0), float(dt), int(what), _ptr(out))
        _lib.check(rc, "uavqp_eval_batch_device")

    def traj_length_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, dt=0.01, length=None, mean_vel=None, n_samples=None):
        """Batched PolyTraj::getTraj + getLength + getMeanVel (poly_traj.hpp:175-207; dt = the reference's 0.01 s): device buffers."""
        rc = _lib.lib().uavqp_traj_length_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), float(dt),
                                                 _ptr(length), _ptr(mean_vel), _ptr(n_samples))
        _lib.check(rc, "uavqp_traj_length_device")

    def time_reallocate_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, v_max, a_max,
                               samples_per_seg=16, max_stretch=1.5, changed=None):
        """One stretch-only time re-allocation step (device buffers, `times` updated in place)."""
        rc = _lib.lib().uavqp_time_reallocate_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                     float(v_max), float(a_max), int(samples_per_seg), float(max_stretch), _ptr(changed))
        _lib.check(rc, "uavqp_time_reallocate_device")

    def cost_time_gradient_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, cost=None, grad=None):
        """uavqp_cost_time_gradient_device: cost [n_traj] = c' P c (integral of the squared r-th derivative, 3 axes) and grad [sum M] =
        d cost / d T_i at the minimiser of the equality-constrained solve (device buffers; either output may be None).  Asynchronous."""
        rc = _lib.lib().uavqp_cost_time_gradient_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), _ptr(cost), _ptr(grad))
        _lib.check(rc, "uavqp_cost_time_gradient_device")

    _DEFAULTS = {}   # c_name -> the library's uavqp_default_<c_name>, looked up once

    @staticmethod
    def _params(struct_cls, c_name, fields):
        """A uavqp_<c_name> struct: uavqp_default_<c_name>, then the fields given (an unknown or reserved one is refused)."""
        default = Context._DEFAULTS.get(c_name)
        if default is None:
            default = Context._DEFAULTS[c_name] = getattr(_lib.lib(), "uavqp_default_" + c_name)
        pp = struct_cls()
        default(ctypes.byref(pp))
        for k, v in fields.items():
            if not hasattr(pp, k) or k in ("struct_size", "reserved_"):
                raise _unknown_field(c_name, k)
            setattr(pp, k, v)
        return pp

    # (the names tests and autograd.py call)
    _limit_params = staticmethod(functools.partial(_params.__func__, _lib.LimitParams, "limit_params"))
    _swarm_params = staticmethod(functools.partial(_params.__func__, _lib.SwarmParams, "swarm_params"))
    _clearance_params = staticmethod(functools.partial(_params.__func__, _lib.ClearanceParams, "clearance_params"))
    _spacetime_params = staticmethod(functools.partial(_params.__func__, _lib.SpacetimeParams, "spacetime_params"))
    _swarm_opt_params = staticmethod(functools.partial(_params.__func__, _lib.SwarmOptParams, "swarm_opt_params"))
    _spacetime_lbfgs_params = staticmethod(functools.partial(_params.__func__, _lib.SpacetimeLbfgsParams, "spacetime_lbfgs_params"))
    _attitude_params = staticmethod(functools.partial(_params.__func__, _lib.AttitudeParams, "attitude_params"))
    _moving_params = staticmethod(functools.partial(_params.__func__, _lib.MovingParams, "moving_params"))

    @staticmethod
    def _solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status):
        """The solved batch of a _host wrapper as contiguous arrays, sizes checked: (seg_offsets or None, times, coeff, status or None,
        n_traj, total segments)."""
        times = np.ascontiguousarray(times, dtype=np.float64).ravel()
        coeff = np.ascontiguousarray(coeff, dtype=np.float64).ravel()
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        so, n_traj, total, _ = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total and coeff.size == 3 * 2 * r * total
        return so, times, coeff, status, n_traj, total

    @staticmethod
    def _swarm_inputs(group_offsets, start, n_traj):
        """(group_offsets or None, n_groups, start or None) of a _host swarm wrapper; no offsets: the whole batch is one swarm."""
        go = None if group_offsets is None else np.ascontiguousarray(group_offsets, dtype=np.int32)
        start = None if start is None else np.ascontiguousarray(start, dtype=np.float64).ravel()
        assert start is None or start.size == n_traj
        return go, (1 if go is None else go.size - 1), start

    def time_optimize_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc,
                             coeff_out, status_out, objective_out, accepted_out=None, **params):
        """uavqp_time_optimize_device on device buffers: `times` holds the start and receives the optimised durations, coeff_out the
        solve at them, objective_out [n_traj][2] f = cost + time_weight * sum T at the start and at the result.
        params: fields of uavqp_time_opt_params that differ from uavqp_default_time_opt_params.  Asynchronous."""
        pp = self._params(_lib.TimeOptParams, "time_opt_params", params)
        rc = _lib.lib().uavqp_time_optimize_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                   _ptr(waypoints), _ptr(times), _ptr(bc), ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out),
                                                   _ptr(objective_out), _ptr(accepted_out))
        _lib.check(rc, "uavqp_time_optimize_device")

    def time_optimize_host(self, r, seg_offsets, waypoints, times, bc, uniform_segments=0, **params):
        """numpy in / numpy out (synchronous).  Returns (times, coeff_flat, status, objective [n_traj][2], accepted)."""
        waypoints = np.ascontiguousarray(waypoints, dtype=np.float64)
        times = np.array(times, dtype=np.float64).ravel()   # a copy: the call updates it in place
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._params(_lib.TimeOptParams, "time_opt_params", params)
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_time_optimize_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                 _ptr(bc), ctypes.byref(pp), _ptr(coeff), _ptr(status), _ptr(objective), _ptr(accepted))
        _lib.check(rc, "uavqp_time_optimize_host")
        return times, coeff, status, objective, accepted

    def limit_penalty_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, status=None, penalty=None, grad_coeff=None,
                             grad_times=None, peak=None, **limits):
        """uavqp_limit_penalty_device on device buffers: the velocity / acceleration limit penalty [n_traj] of solved trajectories, its
        gradient in the coefficients at fixed durations (layout of coeff), its EXPLICIT gradient in the durations at fixed coefficients
        [sum M], and the sampled peaks |v| / v_max, |a| / a_max [n_traj][2]; each output may be None.  status (the solve's, optional):
        trajectories that are not SOLVED get zeros.  limits: fields of uavqp_limit_params that differ from uavqp_default_limit_params.
        Asynchronous."""
        lp = self._limit_params(limits)
        rc = _lib.lib().uavqp_limit_penalty_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), _ptr(status),
                                                   ctypes.byref(lp), _ptr(penalty), _ptr(grad_coeff), _ptr(grad_times), _ptr(peak))
        _lib.check(rc, "uavqp_limit_penalty_device")

    def limit_penalty_host(self, r, seg_offsets, times, coeff, uniform_segments=0, status=None, **limits):
        """numpy in / numpy out (synchronous).  Returns (penalty [n_traj], grad_coeff, grad_times [sum M], peak [n_traj][2])."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        lp = self._limit_params(limits)
        penalty = np.zeros(n_traj, dtype=np.float64)
        g_c = np.zeros_like(coeff)
        g_t = np.zeros(total, dtype=np.float64)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        rc = _lib.lib().uavqp_limit_penalty_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                 ctypes.byref(lp), _ptr(penalty), _ptr(g_c), _ptr(g_t), _ptr(peak))
        _lib.check(rc, "uavqp_limit_penalty_host")
        return penalty, g_c, g_t, peak

    def swarm_penalty_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, n_groups=1, group_offsets=None, start=None,
                             status=None, penalty=None, grad_coeff=None, grad_times=None, grad_start=None, min_sep=None, **params):
        """uavqp_swarm_penalty_device on device buffers: the separation penalty [n_groups] between the vehicles of each swarm (trajectories
        group_offsets[g] .. group_offsets[g + 1]; None with n_groups = 1: the whole batch) compared at the same instants of a shared
        clock, its gradient in the coefficients at fixed durations (layout of coeff), its EXPLICIT gradients in the durations [sum M]
        and in the departure times `start` [n_traj] (None: all zero), and the smallest sampled separation [n_traj]; each output may be
        None.  status (the solve's, optional): vehicles that are not SOLVED are left out of every pair.  params: fields of
        uavqp_swarm_params that differ from uavqp_default_swarm_params (n_samples, clock_start, dt, d_safe, downwash, weight).
        Asynchronous."""
        sp = self._swarm_params(params)
        rc = _lib.lib().uavqp_swarm_penalty_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), _ptr(status),
                                                   int(n_groups), _ptr(group_offsets), _ptr(start), ctypes.byref(sp), _ptr(penalty),
                                                   _ptr(grad_coeff), _ptr(grad_times), _ptr(grad_start), _ptr(min_sep))
        _lib.check(rc, "uavqp_swarm_penalty_device")

    def swarm_penalty_host(self, r, seg_offsets, times, coeff, group_offsets=None, start=None, uniform_segments=0, status=None, **params):
        """numpy in / numpy out (synchronous).  group_offsets None: the whole batch is one swarm.  Returns (penalty [n_groups], grad_coeff,
        grad_times [sum M], grad_start [n_traj], min_sep [n_traj])."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        go, n_groups, start = self._swarm_inputs(group_offsets, start, n_traj)
        sp = self._swarm_params(params)
        penalty = np.zeros(n_groups, dtype=np.float64)
        g_c = np.zeros_like(coeff)
        g_t = np.zeros(total, dtype=np.float64)
        g_s = np.zeros(n_traj, dtype=np.float64)
        min_sep = np.zeros(n_traj, dtype=np.float64)
        rc = _lib.lib().uavqp_swarm_penalty_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                 n_groups, _ptr(go), _ptr(start), ctypes.byref(sp), _ptr(penalty), _ptr(g_c), _ptr(g_t),
                                                 _ptr(g_s), _ptr(min_sep))
        _lib.check(rc, "uavqp_swarm_penalty_host")
        return penalty, g_c, g_t, g_s, min_sep

    def separation_certificate_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, n_groups=1, group_offsets=None, start=None,
                                      status=None, lower_out=None, upper_out=None, where_out=None, verdict_out=None, group_verdict_out=None,
                                      **params):
        """uavqp_separation_certificate_device on device buffers: certified separation between the vehicles of each swarm (described as for
        swarm_penalty_device) over the WHOLE clock window, not at its samples.  lower_out [n_traj] holds for every t of the window and every
        partner, upper_out [n_traj] is taken at a witness, where_out [n_traj][4] int32 = {partner of lower, leaf of lower, partner of upper,
        witness index of upper}, verdict_out [n_traj] and group_verdict_out [n_groups] int32 (_lib.UAVQP_SEPARATION_CERTIFIED / _VIOLATED /
        _MOVING); each may be None.  params: fields of uavqp_separation_params that differ from uavqp_default_separation_params (depth,
        n_cells, clock_start, dt, downwash, d_req).  Asynchronous."""
        sp = self._params(_lib.SeparationParams, "separation_params", params)
        rc = _lib.lib().uavqp_separation_certificate_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                            _ptr(status), int(n_groups), _ptr(group_offsets), _ptr(start), ctypes.byref(sp),
                                                            _ptr(lower_out), _ptr(upper_out), _ptr(where_out), _ptr(verdict_out),
                                                            _ptr(group_verdict_out))
        _lib.check(rc, "uavqp_separation_certificate_device")

    def separation_certificate(self, r, seg_offsets, times, coeff, group_offsets=None, start=None, uniform_segments=0, status=None, **params):
        """uavqp_separation_certificate_host: numpy in / numpy out (synchronous).  group_offsets None: the whole batch is one swarm.  Returns
        (lower [n_traj], upper [n_traj], where [n_traj][4], verdict [n_traj], group_verdict [n_groups]); see separation_certificate_device."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        go, n_groups, start = self._swarm_inputs(group_offsets, start, n_traj)
        sp = self._params(_lib.SeparationParams, "separation_params", params)
        lower = np.zeros(n_traj, dtype=np.float64)
        upper = np.zeros(n_traj, dtype=np.float64)
        where = np.zeros((n_traj, 4), dtype=np.int32)
        verdict = np.zeros(n_traj, dtype=np.int32)
        group_verdict = np.zeros(n_groups, dtype=np.int32)
        rc = _lib.lib().uavqp_separation_certificate_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                          n_groups, _ptr(go), _ptr(start), ctypes.byref(sp), _ptr(lower), _ptr(upper),
                                                          _ptr(where), _ptr(verdict), _ptr(group_verdict))
        _lib.check(rc, "uavqp_separation_certificate_host")
        return lower, upper, where, verdict, group_verdict

    def clearance_penalty_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, esdf, status=None, penalty=None, grad_coeff=None,
                                 grad_times=None, min_dist=None, outside=None, **params):
        """uavqp_clearance_penalty_device on device buffers: the clearance penalty [n_traj] of solved trajectories against the distance
        field `esdf` (an esdf.EsdfMap, updated), its gradient in the coefficients at fixed durations (layout of coeff), its EXPLICIT
        gradient in the durations at fixed coefficients [sum M], the smallest sampled distance [n_traj] and the int32 count of samples
        outside the map [n_traj]; each output may be None.  params: fields of uavqp_clearance_params that differ from the defaults
        (samples_per_seg, d_safe, weight).  Asynchronous."""
        cp = self._clearance_params(params)
        rc = _lib.lib().uavqp_clearance_penalty_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                       _ptr(status), getattr(esdf, "handle", esdf), ctypes.byref(cp), _ptr(penalty),
                                                       _ptr(grad_coeff), _ptr(grad_times), _ptr(min_dist), _ptr(outside))
        _lib.check(rc, "uavqp_clearance_penalty_device")

    def clearance_penalty_host(self, r, seg_offsets, times, coeff, esdf, uniform_segments=0, status=None, **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns (penalty [n_traj], grad_coeff, grad_times [sum M],
        min_dist [n_traj], outside [n_traj] int32)."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        cp = self._clearance_params(params)
        penalty = np.zeros(n_traj, dtype=np.float64)
        g_c = np.zeros_like(coeff)
        g_t = np.zeros(total, dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_clearance_penalty_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                     getattr(esdf, "handle", esdf), ctypes.byref(cp), _ptr(penalty), _ptr(g_c), _ptr(g_t),
                                                     _ptr(min_dist), _ptr(outside))
        _lib.check(rc, "uavqp_clearance_penalty_host")
        return penalty, g_c, g_t, min_dist, outside

    def cost_waypoint_gradient_device(self, r, n_traj, uniform_segments, seg_offsets, coeff, grad, status=None):
        """uavqp_cost_waypoint_gradient_device: grad [sum (M + 1)][3] = d cost / d p_k at the minimiser of the equality-constrained solve,
        all knots of every trajectory, both ends included (device buffers).  status (the solve's, optional): trajectories that are not
        SOLVED get zeros.  Asynchronous."""
        rc = _lib.lib().uavqp_cost_waypoint_gradient_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(coeff), _ptr(status),
                                                            _ptr(grad))
        _lib.check(rc, "uavqp_cost_waypoint_gradient_device")

    def cost_waypoint_gradient_host(self, r, seg_offsets, coeff, uniform_segments=0, status=None):
        """numpy in / numpy out (synchronous).  Returns grad [sum (M + 1)][3]."""
        coeff = np.ascontiguousarray(coeff, dtype=np.float64).ravel()
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        if uniform_segments > 0:
            so, total = None, coeff.size // (3 * 2 * r)
            n_traj = total // uniform_segments
        else:
            so = np.ascontiguousarray(seg_offsets, dtype=np.int32)
            n_traj, total = so.size - 1, int(so[-1])
        assert coeff.size == 3 * 2 * r * total
        grad = np.zeros((total + n_traj, 3), dtype=np.float64)
        rc = _lib.lib().uavqp_cost_waypoint_gradient_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(coeff), _ptr(status), _ptr(grad))
        _lib.check(rc, "uavqp_cost_waypoint_gradient_host")
        return grad

    def waypoint_optimize_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, esdf,
                                 coeff_out, status_out, objective_out, accepted_out=None, min_dist_out=None, outside_out=None, clearance=None,
                                 **params):
        """uavqp_waypoint_optimize_device on device buffers: `waypoints` holds the start and receives the optimised interior waypoints
        (end knots untouched), coeff_out the solve at them, objective_out [n_traj][2] f = smooth_weight * cost + clearance penalty against
        `esdf` (an esdf.EsdfMap, updated) at the start and at the result, min_dist_out / outside_out the penalty's diagnostics at the
        result.  clearance: dict of uavqp_clearance_params fields; params: fields of uavqp_waypoint_opt_params that differ from the
        defaults.  The penalty is soft and the result a local minimum (include/uavqp.h).  Asynchronous."""
        pp = self._params(_lib.WaypointOptParams, "waypoint_opt_params", params)
        cp = self._clearance_params(clearance or {})
        rc = _lib.lib().uavqp_waypoint_optimize_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                       _ptr(waypoints), _ptr(times), _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(cp),
                                                       ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out), _ptr(objective_out),
                                                       _ptr(accepted_out), _ptr(min_dist_out), _ptr(outside_out))
        _lib.check(rc, "uavqp_waypoint_optimize_device")

    def waypoint_optimize_host(self, r, seg_offsets, waypoints, times, bc, esdf, uniform_segments=0, clearance=None, **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns (waypoints [sum (M + 1)][3], coeff_flat, status,
        objective [n_traj][2], accepted, min_dist [n_traj], outside [n_traj] int32)."""
        waypoints = np.array(waypoints, dtype=np.float64).reshape(-1, 3)   # a copy: the call updates it in place
        times = np.ascontiguousarray(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._params(_lib.WaypointOptParams, "waypoint_opt_params", params)
        cp = self._clearance_params(clearance or {})
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_waypoint_optimize_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                     _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(cp), ctypes.byref(pp), _ptr(coeff),
                                                     _ptr(status), _ptr(objective), _ptr(accepted), _ptr(min_dist), _ptr(outside))
        _lib.check(rc, "uavqp_waypoint_optimize_host")
        return waypoints, coeff, status, objective, accepted, min_dist, outside

    def flight_penalty_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, esdf, status=None, penalty=None, grad_coeff=None,
                              grad_times=None, peak=None, min_dist=None, outside=None, limits=None, clearance=None):
        """uavqp_flight_penalty_device on device buffers: limit penalty + clearance penalty against `esdf` (an esdf.EsdfMap, updated) in
        one launch -- the sum [n_traj], its gradient in the coefficients at fixed durations, its EXPLICIT gradient in the durations, and
        the diagnostics of both parts (peak [n_traj][2], min_dist [n_traj], outside [n_traj] int32); each output may be None.  limits /
        clearance: dicts of uavqp_limit_params / uavqp_clearance_params fields that differ from the defaults.  Asynchronous."""
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        rc = _lib.lib().uavqp_flight_penalty_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), _ptr(status),
                                                    getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp), _ptr(penalty),
                                                    _ptr(grad_coeff), _ptr(grad_times), _ptr(peak), _ptr(min_dist), _ptr(outside))
        _lib.check(rc, "uavqp_flight_penalty_device")

    def flight_penalty_host(self, r, seg_offsets, times, coeff, esdf, uniform_segments=0, status=None, limits=None, clearance=None):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns (penalty [n_traj], grad_coeff, grad_times [sum M],
        peak [n_traj][2], min_dist [n_traj], outside [n_traj] int32)."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        penalty = np.zeros(n_traj, dtype=np.float64)
        g_c = np.zeros_like(coeff)
        g_t = np.zeros(total, dtype=np.float64)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_flight_penalty_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                  getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp), _ptr(penalty), _ptr(g_c),
                                                  _ptr(g_t), _ptr(peak), _ptr(min_dist), _ptr(outside))
        _lib.check(rc, "uavqp_flight_penalty_host")
        return penalty, g_c, g_t, peak, min_dist, outside

    def spacetime_optimize_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, esdf,
                                  coeff_out, status_out, objective_out, accepted_out=None, peak_out=None, min_dist_out=None, outside_out=None,
                                  limits=None, clearance=None, **params):
        """uavqp_spacetime_optimize_device on device buffers: `waypoints` and `times` hold the start and receive the jointly optimised
        interior waypoints and durations, coeff_out the solve at them, objective_out [n_traj][2] f = smooth_weight * cost + time_weight *
        sum T + limit penalty + clearance penalty against `esdf` at the start and at the result; peak_out / min_dist_out / outside_out the
        penalties' diagnostics at the result.  limits / clearance: dicts of uavqp_limit_params / uavqp_clearance_params fields; params:
        fields of uavqp_spacetime_params that differ from the defaults.  Both penalties are soft and the result is a local minimum
        (include/uavqp.h).  Asynchronous."""
        pp = self._spacetime_params(params)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        rc = _lib.lib().uavqp_spacetime_optimize_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                        _ptr(waypoints), _ptr(times), _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp),
                                                        ctypes.byref(cp), ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out),
                                                        _ptr(objective_out), _ptr(accepted_out), _ptr(peak_out), _ptr(min_dist_out),
                                                        _ptr(outside_out))
        _lib.check(rc, "uavqp_spacetime_optimize_device")

    def spacetime_optimize_host(self, r, seg_offsets, waypoints, times, bc, esdf, uniform_segments=0, limits=None, clearance=None, **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns (waypoints [sum (M + 1)][3], times [sum M], coeff_flat,
        status, objective [n_traj][2], accepted, peak [n_traj][2], min_dist [n_traj], outside [n_traj] int32)."""
        waypoints = np.array(waypoints, dtype=np.float64).reshape(-1, 3)   # copies: the call updates both in place
        times = np.array(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._spacetime_params(params)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_spacetime_optimize_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                      _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp),
                                                      ctypes.byref(pp), _ptr(coeff), _ptr(status), _ptr(objective), _ptr(accepted), _ptr(peak),
                                                      _ptr(min_dist), _ptr(outside))
        _lib.check(rc, "uavqp_spacetime_optimize_host")
        return waypoints, times, coeff, status, objective, accepted, peak, min_dist, outside

    def swarm_optimize_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, esdf,
                              coeff_out, status_out, objective_out, n_groups=1, group_offsets=None, start=None, accepted_out=None,
                              peak_out=None, min_dist_out=None, outside_out=None, min_sep_out=None, limits=None, clearance=None, swarm=None,
                              **params):
        """uavqp_swarm_optimize_device on device buffers: spacetime_optimize_device with the swarm separation penalty in the objective and
        ONE accept / reject per swarm.  `waypoints`, `times` and (start_window > 0) `start` hold the start and receive the result;
        objective_out [n_groups][2] and accepted_out [n_groups] are per SWARM (trajectories group_offsets[g] .. group_offsets[g + 1]; None
        with n_groups = 1: the whole batch), the diagnostics peak_out / min_dist_out / outside_out / min_sep_out per vehicle.  limits /
        clearance / swarm: dicts of uavqp_limit_params / uavqp_clearance_params / uavqp_swarm_params fields; params: fields of
        uavqp_swarm_opt_params that differ from the defaults.  All penalties are soft and the result is a local minimum (include/uavqp.h).
        Asynchronous."""
        pp = self._swarm_opt_params(params)
        lp, cp, sp = self._limit_params(limits or {}), self._clearance_params(clearance or {}), self._swarm_params(swarm or {})
        rc = _lib.lib().uavqp_swarm_optimize_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                    _ptr(waypoints), _ptr(times), _ptr(bc), int(n_groups), _ptr(group_offsets), _ptr(start),
                                                    getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp), ctypes.byref(sp),
                                                    ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out), _ptr(objective_out),
                                                    _ptr(accepted_out), _ptr(peak_out), _ptr(min_dist_out), _ptr(outside_out),
                                                    _ptr(min_sep_out))
        _lib.check(rc, "uavqp_swarm_optimize_device")

    def swarm_optimize_host(self, r, seg_offsets, waypoints, times, bc, esdf, group_offsets=None, start=None, uniform_segments=0, limits=None,
                            clearance=None, swarm=None, **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  group_offsets None: the whole batch is one swarm; start None:
        all departures zero (and fixed).  Returns (waypoints [sum (M + 1)][3], times [sum M], start [n_traj] or None, coeff_flat, status,
        objective [n_groups][2], accepted [n_groups], peak [n_traj][2], min_dist [n_traj], outside [n_traj] int32, min_sep [n_traj])."""
        waypoints = np.array(waypoints, dtype=np.float64).reshape(-1, 3)   # copies: the call updates all three in place
        times = np.array(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        go = None if group_offsets is None else np.ascontiguousarray(group_offsets, dtype=np.int32)
        n_groups = 1 if go is None else go.size - 1
        start = None if start is None else np.array(start, dtype=np.float64).ravel()
        assert start is None or start.size == n_traj
        pp = self._swarm_opt_params(params)
        lp, cp, sp = self._limit_params(limits or {}), self._clearance_params(clearance or {}), self._swarm_params(swarm or {})
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_groups, 2), dtype=np.float64)
        accepted = np.zeros(n_groups, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        min_sep = np.zeros(n_traj, dtype=np.float64)
        rc = _lib.lib().uavqp_swarm_optimize_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                  _ptr(bc), n_groups, _ptr(go), _ptr(start), getattr(esdf, "handle", esdf), ctypes.byref(lp),
                                                  ctypes.byref(cp), ctypes.byref(sp), ctypes.byref(pp), _ptr(coeff), _ptr(status),
                                                  _ptr(objective), _ptr(accepted), _ptr(peak), _ptr(min_dist), _ptr(outside), _ptr(min_sep))
        _lib.check(rc, "uavqp_swarm_optimize_host")
        return waypoints, times, start, coeff, status, objective, accepted, peak, min_dist, outside, min_sep

    def spacetime_lbfgs_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, esdf,
                               coeff_out, status_out, objective_out, accepted_out=None, peak_out=None, min_dist_out=None, outside_out=None,
                               limits=None, clearance=None, **params):
        """uavqp_spacetime_lbfgs_device on device buffers: spacetime_optimize_device with limited-memory BFGS directions kept per
        trajectory on the device -- the same objective, bounds, arguments and outputs, fewer trials to the same objective.  params: fields
        of uavqp_spacetime_lbfgs_params that differ from the defaults (memory, max_backtracks and curvature_eps besides those of
        uavqp_spacetime_params).  Asynchronous."""
        pp = self._spacetime_lbfgs_params(params)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        rc = _lib.lib().uavqp_spacetime_lbfgs_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                     _ptr(waypoints), _ptr(times), _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp),
                                                     ctypes.byref(cp), ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out), _ptr(objective_out),
                                                     _ptr(accepted_out), _ptr(peak_out), _ptr(min_dist_out), _ptr(outside_out))
        _lib.check(rc, "uavqp_spacetime_lbfgs_device")

    def spacetime_lbfgs_host(self, r, seg_offsets, waypoints, times, bc, esdf, uniform_segments=0, limits=None, clearance=None, **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns what spacetime_optimize_host returns."""
        waypoints = np.array(waypoints, dtype=np.float64).reshape(-1, 3)   # copies: the call updates both in place
        times = np.array(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._spacetime_lbfgs_params(params)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_spacetime_lbfgs_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                   _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp), ctypes.byref(pp),
                                                   _ptr(coeff), _ptr(status), _ptr(objective), _ptr(accepted), _ptr(peak), _ptr(min_dist),
                                                   _ptr(outside))
        _lib.check(rc, "uavqp_spacetime_lbfgs_host")
        return waypoints, times, coeff, status, objective, accepted, peak, min_dist, outside

    def attitude_penalty_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, status=None, penalty=None, grad_coeff=None,
                                grad_times=None, peak=None, **params):
        """uavqp_attitude_penalty_device on device buffers: the thrust / tilt / body-rate penalty [n_traj] of solved trajectories, its
        gradient in the coefficients at fixed durations (layout of coeff), its EXPLICIT gradient in the durations at fixed coefficients
        [sum M], and the sampled peaks [n_traj][4] (largest and smallest specific thrust in m/s^2, largest tilt in rad, largest body rate
        in rad/s); each output may be None.  status (the solve's, optional): trajectories that are not SOLVED get zeros.  params: fields
        of uavqp_attitude_params that differ from uavqp_default_attitude_params.  Asynchronous."""
        ap = self._attitude_params(params)
        rc = _lib.lib().uavqp_attitude_penalty_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                      _ptr(status), ctypes.byref(ap), _ptr(penalty), _ptr(grad_coeff), _ptr(grad_times),
                                                      _ptr(peak))
        _lib.check(rc, "uavqp_attitude_penalty_device")

    def attitude_penalty_host(self, r, seg_offsets, times, coeff, uniform_segments=0, status=None, **params):
        """numpy in / numpy out (synchronous).  Returns (penalty [n_traj], grad_coeff, grad_times [sum M], peak [n_traj][4])."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        ap = self._attitude_params(params)
        penalty = np.zeros(n_traj, dtype=np.float64)
        g_c = np.zeros_like(coeff)
        g_t = np.zeros(total, dtype=np.float64)
        peak = np.zeros((n_traj, 4), dtype=np.float64)
        rc = _lib.lib().uavqp_attitude_penalty_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                    ctypes.byref(ap), _ptr(penalty), _ptr(g_c), _ptr(g_t), _ptr(peak))
        _lib.check(rc, "uavqp_attitude_penalty_host")
        return penalty, g_c, g_t, peak

    def envelope_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, status=None, box_lo=None, box_hi=None, range_out=None,
                        norm_out=None, peak_out=None, seg_verdict_out=None, verdict_out=None, **params):
        """uavqp_envelope_device on device buffers: certified bounds of solved trajectories over whole segments.  range_out
        [sum M][4][3][4] (derivative order, axis, (outer_lo, inner_lo, inner_hi, outer_hi)), norm_out [sum M][5][4] (|v|, |a|, |j|, specific
        thrust, tilt polynomial w), peak_out [n_traj][5][4], seg_verdict_out [sum M] and verdict_out [n_traj] (int32: bit 2k certified,
        bit 2k + 1 violated, k indexing _lib.ENVELOPE_TESTS); each may be None.  box_lo / box_hi [sum M][3]: one box per segment, both or
        neither.  params: fields of uavqp_envelope_params (depth, v_max, a_max, j_max, f_min, f_max, tilt_max; a limit of 0 is off).
        Asynchronous."""
        ep = self._params(_lib.EnvelopeParams, "envelope_params", params)
        rc = _lib.lib().uavqp_envelope_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), _ptr(status),
                                              ctypes.byref(ep), _ptr(box_lo), _ptr(box_hi), _ptr(range_out), _ptr(norm_out), _ptr(peak_out),
                                              _ptr(seg_verdict_out), _ptr(verdict_out))
        _lib.check(rc, "uavqp_envelope_device")

    def envelope(self, r, seg_offsets, times, coeff, uniform_segments=0, status=None, box_lo=None, box_hi=None, **params):
        """uavqp_envelope_host: numpy in / numpy out (synchronous).  Returns (range [sum M][4][3][4], norm [sum M][5][4],
        peak [n_traj][5][4], seg_verdict [sum M], verdict [n_traj]); see envelope_device."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        if box_lo is not None:
            box_lo = np.ascontiguousarray(box_lo, dtype=np.float64).reshape(total, 3)
        if box_hi is not None:
            box_hi = np.ascontiguousarray(box_hi, dtype=np.float64).reshape(total, 3)
        ep = self._params(_lib.EnvelopeParams, "envelope_params", params)
        rng = np.zeros((total, 4, 3, 4), dtype=np.float64)
        norm = np.zeros((total, 5, 4), dtype=np.float64)
        peak = np.zeros((n_traj, 5, 4), dtype=np.float64)
        seg_verdict = np.zeros(total, dtype=np.int32)
        verdict = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_envelope_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                            ctypes.byref(ep), _ptr(box_lo), _ptr(box_hi), _ptr(rng), _ptr(norm), _ptr(peak), _ptr(seg_verdict),
                                            _ptr(verdict))
        _lib.check(rc, "uavqp_envelope_host")
        return rng, norm, peak, seg_verdict, verdict

    def clearance_certificate_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, esdf, status=None, clear_out=None,
                                     witness_out=None, peak_out=None, seg_verdict_out=None, verdict_out=None, **params):
        """uavqp_clearance_certificate_device on device buffers: certified clearance of solved trajectories against the distance field
        `esdf` (an EsdfMap, updated) over whole segments.  clear_out [sum M][2] (lower: holds for ALL t; upper: taken at the witness),
        witness_out [sum M] (int32 l: the witness is at t = l T_i / 2^depth), peak_out [n_traj][2] (the smallest lower / upper of the
        trajectory), seg_verdict_out [sum M] and verdict_out [n_traj] (int32: _lib.UAVQP_CLEARANCE_CERTIFIED / _VIOLATED / _OUTSIDE); each
        may be None.  params: depth (0..8, default 4), d_req (m, default 0.5).  Asynchronous."""
        cp = self._params(_lib.ClearanceCertParams, "clearance_cert_params", params)
        rc = _lib.lib().uavqp_clearance_certificate_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                           _ptr(status), getattr(esdf, "handle", esdf), ctypes.byref(cp), _ptr(clear_out),
                                                           _ptr(witness_out), _ptr(peak_out), _ptr(seg_verdict_out), _ptr(verdict_out))
        _lib.check(rc, "uavqp_clearance_certificate_device")

    def clearance_certificate(self, r, seg_offsets, times, coeff, esdf, uniform_segments=0, status=None, **params):
        """uavqp_clearance_certificate_host: numpy in / numpy out (synchronous; the map stays on the device).  Returns (clear [sum M][2],
        witness [sum M], peak [n_traj][2], seg_verdict [sum M], verdict [n_traj]); see clearance_certificate_device."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        cp = self._params(_lib.ClearanceCertParams, "clearance_cert_params", params)
        clear = np.zeros((total, 2), dtype=np.float64)
        witness = np.zeros(total, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        seg_verdict = np.zeros(total, dtype=np.int32)
        verdict = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_clearance_certificate_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                         getattr(esdf, "handle", esdf), ctypes.byref(cp), _ptr(clear), _ptr(witness), _ptr(peak),
                                                         _ptr(seg_verdict), _ptr(verdict))
        _lib.check(rc, "uavqp_clearance_certificate_host")
        return clear, witness, peak, seg_verdict, verdict

    def attitude_optimize_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, esdf,
                                 coeff_out, status_out, objective_out, accepted_out=None, peak_out=None, min_dist_out=None, outside_out=None,
                                 attitude_peak_out=None, limits=None, clearance=None, attitude=None, **params):
        """uavqp_attitude_optimize_device on device buffers: spacetime_lbfgs_device with the attitude penalty inside the objective
        (objective_out includes it); attitude_peak_out [n_traj][4] receives attitude_penalty_device's peaks at the result.  attitude: dict
        of uavqp_attitude_params fields; everything else as spacetime_lbfgs_device.  Asynchronous."""
        pp = self._spacetime_lbfgs_params(params)
        lp, cp, ap = self._limit_params(limits or {}), self._clearance_params(clearance or {}), self._attitude_params(attitude or {})
        rc = _lib.lib().uavqp_attitude_optimize_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                       _ptr(waypoints), _ptr(times), _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp),
                                                       ctypes.byref(cp), ctypes.byref(ap), ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out),
                                                       _ptr(objective_out), _ptr(accepted_out), _ptr(peak_out), _ptr(min_dist_out),
                                                       _ptr(outside_out), _ptr(attitude_peak_out))
        _lib.check(rc, "uavqp_attitude_optimize_device")

    def attitude_optimize_host(self, r, seg_offsets, waypoints, times, bc, esdf, uniform_segments=0, limits=None, clearance=None, attitude=None,
                               **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns what spacetime_lbfgs_host returns, and the attitude
        peaks [n_traj][4] after it."""
        waypoints = np.array(waypoints, dtype=np.float64).reshape(-1, 3)   # copies: the call updates both in place
        times = np.array(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._spacetime_lbfgs_params(params)
        lp, cp, ap = self._limit_params(limits or {}), self._clearance_params(clearance or {}), self._attitude_params(attitude or {})
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        attitude_peak = np.zeros((n_traj, 4), dtype=np.float64)
        rc = _lib.lib().uavqp_attitude_optimize_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                     _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp), ctypes.byref(ap),
                                                     ctypes.byref(pp), _ptr(coeff), _ptr(status), _ptr(objective), _ptr(accepted), _ptr(peak),
                                                     _ptr(min_dist), _ptr(outside), _ptr(attitude_peak))
        _lib.check(rc, "uavqp_attitude_optimize_host")
        return waypoints, times, coeff, status, objective, accepted, peak, min_dist, outside, attitude_peak

    _MOVING_POINTERS = ("seg_offsets", "times", "coeff", "start", "radius", "set_offsets", "traj_set", "traj_start")

    @classmethod
    def _moving_obstacles(cls, obstacles):
        """uavqp_moving_obstacles from a dict: n_obs, uniform_segments (0: ragged), n_sets (default 1) and the arrays of
        _MOVING_POINTERS (numpy arrays, torch tensors or raw addresses; absent or None: NULL).  The arrays must outlive the call."""
        mo = _lib.MovingObstacles()
        mo.struct_size = ctypes.sizeof(_lib.MovingObstacles)
        for k in obstacles:
            if k not in cls._MOVING_POINTERS and k not in ("n_obs", "uniform_segments", "n_sets"):
                raise _unknown_field("moving_obstacles", k)
        mo.n_obs = int(obstacles.get("n_obs", 0))
        mo.uniform_segments = int(obstacles.get("uniform_segments", 0))
        mo.n_sets = int(obstacles.get("n_sets", 1))
        for k in cls._MOVING_POINTERS:
            setattr(mo, k, _ptr(obstacles.get(k)))
        return mo

    @classmethod
    def _moving_obstacles_host(cls, r, obstacles, n_traj):
        """The same from host arrays, shapes checked: times [sum Mo], coeff (layout of a batch's coeff), seg_offsets or uniform_segments,
        start / radius [n_obs], set_offsets [n_sets + 1], traj_set / traj_start [n_traj].  Returns (struct, the arrays it points into)."""
        for k in obstacles:
            if k not in cls._MOVING_POINTERS and k not in ("uniform_segments",):
                raise ValueError(f"unknown moving-obstacle field {k!r}")
        def arr(k, dt):
            v = obstacles.get(k)
            return None if v is None else np.ascontiguousarray(v, dtype=dt).ravel()
        keep = {k: arr(k, np.int32 if k in ("seg_offsets", "set_offsets", "traj_set") else np.float64) for k in cls._MOVING_POINTERS}
        uni = int(obstacles.get("uniform_segments", 0))
        times = keep["times"] if keep["times"] is not None else np.zeros(0)
        so, n_obs, total, _ = _batch_shape(keep["seg_offsets"], times, uni) if (uni > 0 or keep["seg_offsets"] is not None) else (None, 0, 0, 1)
        keep["seg_offsets"] = so
        assert times.size == total and (keep["coeff"] is None or keep["coeff"].size == 3 * 2 * r * total)
        for k in ("start", "radius"):
            assert keep[k] is None or keep[k].size == n_obs, k
        for k in ("traj_set", "traj_start"):
            assert keep[k] is None or keep[k].size == n_traj, k
        d = dict(keep, n_obs=n_obs, uniform_segments=uni, n_sets=1 if keep["set_offsets"] is None else keep["set_offsets"].size - 1)
        return cls._moving_obstacles(d), keep

    def moving_penalty_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, obstacles, status=None, penalty=None,
                              grad_coeff=None, grad_times=None, grad_start=None, min_gap=None, nearest=None, **params):
        """uavqp_moving_penalty_device on device buffers: the penalty [n_traj] of solved trajectories against MOVING obstacle tracks, its
        gradient in the coefficients at fixed durations (layout of coeff), its EXPLICIT gradients in the durations [sum M] and in the
        departure [n_traj], the smallest sampled gap [n_traj] and the obstacle that attains it [n_traj] int32; each output may be None.
        obstacles: dict of uavqp_moving_obstacles (n_obs, uniform_segments, n_sets and the device arrays seg_offsets, times, coeff, start,
        radius, set_offsets, traj_set, traj_start).  params: fields of uavqp_moving_params that differ from uavqp_default_moving_params
        (samples_per_seg, d_safe, downwash, weight).  Asynchronous."""
        mp = self._moving_params(params)
        mo = self._moving_obstacles(obstacles)
        rc = _lib.lib().uavqp_moving_penalty_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff), _ptr(status),
                                                    ctypes.byref(mo), ctypes.byref(mp), _ptr(penalty), _ptr(grad_coeff), _ptr(grad_times),
                                                    _ptr(grad_start), _ptr(min_gap), _ptr(nearest))
        _lib.check(rc, "uavqp_moving_penalty_device")

    def moving_penalty_host(self, r, seg_offsets, times, coeff, obstacles, uniform_segments=0, status=None, **params):
        """numpy in / numpy out (synchronous).  obstacles: dict of host arrays (_moving_obstacles_host).  Returns (penalty [n_traj],
        grad_coeff, grad_times [sum M], grad_start [n_traj], min_gap [n_traj], nearest [n_traj])."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        mp = self._moving_params(params)
        mo, keep = self._moving_obstacles_host(r, obstacles, n_traj)
        penalty = np.zeros(n_traj, dtype=np.float64)
        g_c = np.zeros_like(coeff)
        g_t = np.zeros(total, dtype=np.float64)
        g_s = np.zeros(n_traj, dtype=np.float64)
        min_gap = np.zeros(n_traj, dtype=np.float64)
        nearest = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_moving_penalty_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                  ctypes.byref(mo), ctypes.byref(mp), _ptr(penalty), _ptr(g_c), _ptr(g_t), _ptr(g_s),
                                                  _ptr(min_gap), _ptr(nearest))
        del keep
        _lib.check(rc, "uavqp_moving_penalty_host")
        return penalty, g_c, g_t, g_s, min_gap, nearest

    def moving_optimize_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, esdf,
                               obstacles, coeff_out, status_out, objective_out, accepted_out=None, peak_out=None, min_dist_out=None,
                               outside_out=None, attitude_peak_out=None, min_gap_out=None, nearest_out=None, limits=None, clearance=None,
                               attitude=None, moving=None, **params):
        """uavqp_moving_optimize_device on device buffers: attitude_optimize_device with the moving-obstacle penalty inside the objective
        (objective_out includes it); min_gap_out [n_traj] / nearest_out [n_traj] int32 receive moving_penalty_device's at the result.
        obstacles as for moving_penalty_device; moving: dict of uavqp_moving_params fields; attitude: dict of uavqp_attitude_params
        fields, None: NO attitude term; everything else as spacetime_lbfgs_device.  Asynchronous."""
        pp = self._spacetime_lbfgs_params(params)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        ap = None if attitude is None else self._attitude_params(attitude)
        mp, mo = self._moving_params(moving or {}), self._moving_obstacles(obstacles)
        rc = _lib.lib().uavqp_moving_optimize_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                     _ptr(waypoints), _ptr(times), _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp),
                                                     ctypes.byref(cp), None if ap is None else ctypes.byref(ap), ctypes.byref(mo),
                                                     ctypes.byref(mp), ctypes.byref(pp), _ptr(coeff_out), _ptr(status_out), _ptr(objective_out),
                                                     _ptr(accepted_out), _ptr(peak_out), _ptr(min_dist_out), _ptr(outside_out),
                                                     _ptr(attitude_peak_out), _ptr(min_gap_out), _ptr(nearest_out))
        _lib.check(rc, "uavqp_moving_optimize_device")

    def moving_optimize_host(self, r, seg_offsets, waypoints, times, bc, esdf, obstacles, uniform_segments=0, limits=None, clearance=None,
                             attitude=None, moving=None, **params):
        """numpy in / numpy out (synchronous; the map stays on the device).  Returns what attitude_optimize_host returns (the attitude
        peaks are zeros when attitude is None), then min_gap [n_traj] and nearest [n_traj]."""
        waypoints = np.array(waypoints, dtype=np.float64).reshape(-1, 3)   # copies: the call updates both in place
        times = np.array(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._spacetime_lbfgs_params(params)
        lp, cp = self._limit_params(limits or {}), self._clearance_params(clearance or {})
        ap = None if attitude is None else self._attitude_params(attitude)
        mp = self._moving_params(moving or {})
        mo, keep = self._moving_obstacles_host(r, obstacles, n_traj)
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        min_dist = np.zeros(n_traj, dtype=np.float64)
        outside = np.zeros(n_traj, dtype=np.int32)
        attitude_peak = np.zeros((n_traj, 4), dtype=np.float64)
        min_gap = np.zeros(n_traj, dtype=np.float64)
        nearest = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_moving_optimize_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                   _ptr(bc), getattr(esdf, "handle", esdf), ctypes.byref(lp), ctypes.byref(cp),
                                                   None if ap is None else ctypes.byref(ap), ctypes.byref(mo), ctypes.byref(mp),
                                                   ctypes.byref(pp), _ptr(coeff), _ptr(status), _ptr(objective), _ptr(accepted), _ptr(peak),
                                                   _ptr(min_dist), _ptr(outside), _ptr(attitude_peak), _ptr(min_gap), _ptr(nearest))
        del keep
        _lib.check(rc, "uavqp_moving_optimize_host")
        return waypoints, times, coeff, status, objective, accepted, peak, min_dist, outside, attitude_peak, min_gap, nearest

    def moving_certificate_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, obstacles, status=None, gap_out=None,
                                  where_out=None, peak_out=None, seg_verdict_out=None, verdict_out=None, **params):
        """uavqp_moving_certificate_device on device buffers: the certified gap of every segment to the obstacle tracks of its trajectory's
        set (obstacles: the dict moving_penalty_device takes) for EVERY t of the segment, not at samples.  gap_out [sum M][2] = lower (holds
        for all t), upper (taken at a witness); where_out [sum M][4] int32 = {obstacle of lower, leaf of lower, obstacle of upper, witness
        index of upper}; peak_out [n_traj][2] their minima over the segments; seg_verdict_out [sum M] and verdict_out [n_traj] int32
        (_lib.UAVQP_MOVING_CERT_CERTIFIED / _VIOLATED); each may be None.  params: fields of uavqp_moving_cert_params that differ from
        uavqp_default_moving_cert_params (depth, downwash, d_req).  Asynchronous."""
        cp = self._params(_lib.MovingCertParams, "moving_cert_params", params)
        mo = self._moving_obstacles(obstacles)
        rc = _lib.lib().uavqp_moving_certificate_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                        _ptr(status), ctypes.byref(mo), ctypes.byref(cp), _ptr(gap_out), _ptr(where_out),
                                                        _ptr(peak_out), _ptr(seg_verdict_out), _ptr(verdict_out))
        _lib.check(rc, "uavqp_moving_certificate_device")

    def moving_certificate_host(self, r, seg_offsets, times, coeff, obstacles, uniform_segments=0, status=None, **params):
        """uavqp_moving_certificate_host: numpy in / numpy out (synchronous).  obstacles: dict of host arrays (_moving_obstacles_host).
        Returns (gap [sum M][2], where [sum M][4], peak [n_traj][2], seg_verdict [sum M], verdict [n_traj]); see
        moving_certificate_device."""
        so, times, coeff, status, n_traj, total = self._solved_inputs(r, seg_offsets, times, coeff, uniform_segments, status)
        cp = self._params(_lib.MovingCertParams, "moving_cert_params", params)
        mo, keep = self._moving_obstacles_host(r, obstacles, n_traj)
        gap = np.zeros((total, 2), dtype=np.float64)
        where = np.zeros((total, 4), dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        seg_verdict = np.zeros(total, dtype=np.int32)
        verdict = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_moving_certificate_host(self._h, r, n_traj, uniform_segments, _ptr(so), _ptr(times), _ptr(coeff), _ptr(status),
                                                      ctypes.byref(mo), ctypes.byref(cp), _ptr(gap), _ptr(where), _ptr(peak),
                                                      _ptr(seg_verdict), _ptr(verdict))
        del keep
        _lib.check(rc, "uavqp_moving_certificate_host")
        return gap, where, peak, seg_verdict, verdict

    def time_optimize_limits_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc,
                                    coeff_out, status_out, objective_out, accepted_out=None, peak_out=None, limits=None, **params):
        """uavqp_time_optimize_limits_device on device buffers: time_optimize_device with the limit penalty inside the objective
        (objective_out includes it); peak_out [n_traj][2] receives the sampled |v| / v_max, |a| / a_max at the result.  limits: dict of
        uavqp_limit_params fields; params: fields of uavqp_time_opt_params.  The penalty is soft (include/uavqp.h).  Asynchronous."""
        pp = self._params(_lib.TimeOptParams, "time_opt_params", params)
        lp = self._limit_params(limits or {})
        rc = _lib.lib().uavqp_time_optimize_limits_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments),
                                                          _ptr(seg_offsets), _ptr(waypoints), _ptr(times), _ptr(bc), ctypes.byref(pp),
                                                          _ptr(coeff_out), _ptr(status_out), _ptr(objective_out), _ptr(accepted_out),
                                                          ctypes.byref(lp), _ptr(peak_out))
        _lib.check(rc, "uavqp_time_optimize_limits_device")

    def time_optimize_limits_host(self, r, seg_offsets, waypoints, times, bc, limits, uniform_segments=0, **params):
        """numpy in / numpy out (synchronous).  Returns (times, coeff_flat, status, objective [n_traj][2], accepted, peak [n_traj][2])."""
        waypoints = np.ascontiguousarray(waypoints, dtype=np.float64)
        times = np.array(times, dtype=np.float64).ravel()   # a copy: the call updates it in place
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        pp = self._params(_lib.TimeOptParams, "time_opt_params", params)
        lp = self._limit_params(limits)
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        objective = np.zeros((n_traj, 2), dtype=np.float64)
        accepted = np.zeros(n_traj, dtype=np.int32)
        peak = np.zeros((n_traj, 2), dtype=np.float64)
        rc = _lib.lib().uavqp_time_optimize_limits_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                        _ptr(bc), ctypes.byref(pp), _ptr(coeff), _ptr(status), _ptr(objective), _ptr(accepted),
                                                        ctypes.byref(lp), _ptr(peak))
        _lib.check(rc, "uavqp_time_optimize_limits_host")
        return times, coeff, status, objective, accepted, peak

    def solve_backward_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc, coeff,
                              grad_coeff, grad_times=None, grad_waypoints=None, grad_bc=None, status=None):
        """uavqp_solve_backward_device on device buffers: for grad_coeff = dPhi/dcoeff (layout of coeff) the vector-Jacobian products
        through the minimiser of uavqp_solve_batch_device -- grad_times [sum M], grad_waypoints [sum (M + 1)][3], grad_bc
        [n_traj][2][r-1][3]; each output may be None.  status (the solve's, optional): trajectories that are not SOLVED get zeros.
        The explicit dependence of the caller's loss on the durations is not included.  Asynchronous."""
        rc = _lib.lib().uavqp_solve_backward_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                    _ptr(waypoints), _ptr(times), _ptr(bc), _ptr(coeff), _ptr(status), _ptr(grad_coeff),
                                                    _ptr(grad_times), _ptr(grad_waypoints), _ptr(grad_bc))
        _lib.check(rc, "uavqp_solve_backward_device")

    def solve_backward_host(self, r, seg_offsets, waypoints, times, bc, coeff, grad_coeff, uniform_segments=0, status=None,
                            want=(True, True, True)):
        """numpy in / numpy out (synchronous).  Returns (grad_times, grad_waypoints, grad_bc); an entry of `want` that is False gives None."""
        waypoints = np.ascontiguousarray(waypoints, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64).ravel()
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        coeff = np.ascontiguousarray(coeff, dtype=np.float64).ravel()
        grad_coeff = np.ascontiguousarray(grad_coeff, dtype=np.float64).ravel()
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert times.size == total and waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3 and coeff.size == 3 * 2 * r * total == grad_coeff.size
        g_t = np.zeros(total, dtype=np.float64) if want[0] else None
        g_w = np.zeros((total + n_traj, 3), dtype=np.float64) if want[1] else None
        g_b = np.zeros((n_traj, 2, r - 1, 3), dtype=np.float64) if want[2] else None
        rc = _lib.lib().uavqp_solve_backward_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                  _ptr(bc), _ptr(coeff), _ptr(status), _ptr(grad_coeff), _ptr(g_t), _ptr(g_w), _ptr(g_b))
        _lib.check(rc, "uavqp_solve_backward_host")
        return g_t, g_w, g_b

    def ellipsoid_check_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, n_samples, t0, dt,
                               obstacles, n_obs, robot_r, robot_h, first_hit, flags=None):
        """Batched KinoAstar::isCollisionFree over the samples of solved trajectories (device buffers)."""
        rc = _lib.lib().uavqp_ellipsoid_check_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                     n_samples, float(t0), float(dt), _ptr(obstacles), int(n_obs),
                                                     float(robot_r), float(robot_h), _ptr(first_hit), _ptr(flags))
        _lib.check(rc, "uavqp_ellipsoid_check_device")

    def solve_corridor_device(self, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, corr_lo, corr_hi,
                              coeff_out, status_out, iters_out=None, active_set=None, warm_start=False):
        """Corridor-constrained solve on device buffers; active_set ([n_traj,3,2] int64/uint64 device tensor) carries the
        working set between the re-solves of an outer loop (warm_start=True reads it; warm_start=2 also starts the free positions from
        the polynomials found in coeff_out -- include/uavqp.h)."""
        rc = _lib.lib().uavqp_solve_corridor_warm_device(self._h, r, n_traj, uniform_segments, max_segments, _ptr(seg_offsets), _ptr(waypoints),
                                                         _ptr(times), _ptr(bc), _ptr(corr_lo), _ptr(corr_hi), _ptr(coeff_out), _ptr(status_out),
                                                         _ptr(iters_out), _ptr(active_set), int(warm_start))
        _lib.check(rc, "uavqp_solve_corridor_warm_device")

    def solve_rows_device(self, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, corr_lo, corr_hi,
                          rows_per_segment, row_tau, row_deriv, row_lo, row_hi, coeff_out, status_out, iters_out=None, active_out=None):
        """Knot boxes (or None: waypoint equalities) + up to rows_per_segment general rows lo <= p_i^(d)(tau T_i) <= hi per segment and
        axis; exact dual active-set solve on device buffers (uavqp_solve_rows_batch_device)."""
        rc = _lib.lib().uavqp_solve_rows_batch_device(self._h, r, n_traj, uniform_segments, max_segments, _ptr(seg_offsets), _ptr(waypoints),
                                                      _ptr(times), _ptr(bc), _ptr(corr_lo), _ptr(corr_hi), int(rows_per_segment), _ptr(row_tau),
                                                      _ptr(row_deriv), _ptr(row_lo), _ptr(row_hi), _ptr(coeff_out), _ptr(status_out), _ptr(iters_out),
                                                      _ptr(active_out))
        _lib.check(rc, "uavqp_solve_rows_batch_device")

    def corridor_from_cloud_device(self, r, n_traj, uniform_segments, seg_offsets, n_rows, waypoints, times, coeff,
                                   obstacles, n_obs, robot_r, robot_h, h_max, corr_lo, corr_hi, clearance=None):
        """Corridor boxes of every waypoint row from an obstacle cloud, robot ellipsoid of kino_astar.cpp:721-758
        (device buffers; coeff/times None = hover attitude)."""
        rc = _lib.lib().uavqp_corridor_from_cloud_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), int(n_rows),
                                                         _ptr(waypoints), _ptr(times), _ptr(coeff), _ptr(obstacles), int(n_obs),
                                                         float(robot_r), float(robot_h), float(h_max), _ptr(corr_lo), _ptr(corr_hi),
                                                         _ptr(clearance))
        _lib.check(rc, "uavqp_corridor_from_cloud_device")

    def obstacle_grid_build(self, obstacles, n_obs, cell_size):
        """Uniform grid over a device point cloud; returns an opaque handle (free it with obstacle_grid_destroy)."""
        h = ctypes.c_void_p()
        rc = _lib.lib().uavqp_obstacle_grid_build_device(self._h, _ptr(obstacles),
                                                         int(n_obs), float(cell_size), ctypes.byref(h))
        _lib.check(rc, "uavqp_obstacle_grid_build_device")
        return h

    def obstacle_grid_destroy(self, grid):
        _lib.check(_lib.lib().uavqp_obstacle_grid_destroy(self._h, grid), "uavqp_obstacle_grid_destroy")

    def ellipsoid_check_grid_device(self, r, n_traj, uniform_segments, seg_offsets, times, coeff, n_samples, t0, dt,
                                    grid, robot_r, robot_h, first_hit, flags=None):
        """ellipsoid_check_device with the candidates taken from an obstacle grid (identical flags, no exhaustive scan)."""
        rc = _lib.lib().uavqp_ellipsoid_check_grid_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(times), _ptr(coeff),
                                                          n_samples, float(t0), float(dt), grid, float(robot_r), float(robot_h),
                                                          _ptr(first_hit), _ptr(flags))
        _lib.check(rc, "uavqp_ellipsoid_check_grid_device")

    def corridor_pipeline_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc,
                                 obstacles, n_obs, coeff_out, status_out, corr_lo, corr_hi, first_hit=None, grid=None, **params):
        """uavqp_corridor_pipeline_device: BASELINE config 5 as one C-ABI call on device buffers (times is stretched in place).
        params: fields of uavqp_pipeline_params that differ from uavqp_default_pipeline_params.  Returns the uavqp_pipeline_result
        fields as a dict (repair_rows is 0: the box repair places no rows).  Synchronous."""
        pp = self._params(_lib.PipelineParams, "pipeline_params", params)
        res = _lib.PipelineResult()
        rc = _lib.lib().uavqp_corridor_pipeline_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                       _ptr(waypoints), _ptr(times), _ptr(bc), _ptr(obstacles), int(n_obs), grid, ctypes.byref(pp),
                                                       _ptr(coeff_out), _ptr(status_out), _ptr(corr_lo), _ptr(corr_hi), _ptr(first_hit), ctypes.byref(res))
        _lib.check(rc, "uavqp_corridor_pipeline_device")
        return {k: getattr(res, k) for k, _ in _lib.PipelineResult._fields_}

    def corridor_pipeline_rows_device(self, r, n_traj, uniform_segments, max_segments, total_segments, seg_offsets, waypoints, times, bc,
                                      obstacles, n_obs, coeff_out, status_out, corr_lo, corr_hi, row_tau, row_deriv, row_lo, row_hi,
                                      first_hit=None, grid=None, **params):
        """uavqp_corridor_pipeline_rows_device: corridor_pipeline_device with the rows repair (between-knot hits become position rows,
        knot boxes stay).  row_tau / row_deriv [total_segments, 2], row_lo / row_hi [total_segments, 2, 3] device buffers: set to unused
        by the call, on return the rows of the final solve.  Returns the uavqp_pipeline_result fields as a dict.  Synchronous."""
        pp = self._params(_lib.PipelineParams, "pipeline_params", params)
        res = _lib.PipelineResult()
        rc = _lib.lib().uavqp_corridor_pipeline_rows_device(self._h, r, n_traj, uniform_segments, max_segments, int(total_segments), _ptr(seg_offsets),
                                                            _ptr(waypoints), _ptr(times), _ptr(bc), _ptr(obstacles), int(n_obs), grid, ctypes.byref(pp),
                                                            _ptr(coeff_out), _ptr(status_out), _ptr(corr_lo), _ptr(corr_hi), _ptr(first_hit), _ptr(row_tau),
                                                            _ptr(row_deriv), _ptr(row_lo), _ptr(row_hi), ctypes.byref(res))
        _lib.check(rc, "uavqp_corridor_pipeline_rows_device")
        return {k: getattr(res, k) for k, _ in _lib.PipelineResult._fields_}

    def repair_rows_from_hits_device(self, r, n_traj, uniform_segments, seg_offsets, waypoints, times, coeff, n_samples, t0, dt, flags,
                                     obstacles, n_obs, robot_r, robot_h, h_max, row_tau, row_deriv, row_lo, row_hi, new_rows):
        """uavqp_repair_rows_from_hits_device: position rows around pushed-out anchors for the colliding runs of a check's per-sample
        flags ([n_traj, n_samples] uint8).  Row arrays IN / OUT in the rows_per_segment = 2 layout; new_rows [n_traj] int32 OUT.
        Device buffers, asynchronous."""
        rc = _lib.lib().uavqp_repair_rows_from_hits_device(self._h, r, n_traj, uniform_segments, _ptr(seg_offsets), _ptr(waypoints), _ptr(times),
                                                           _ptr(coeff), int(n_samples), float(t0), float(dt), _ptr(flags), _ptr(obstacles), int(n_obs),
                                                           float(robot_r), float(robot_h), float(h_max), _ptr(row_tau), _ptr(row_deriv), _ptr(row_lo),
                                                           _ptr(row_hi), _ptr(new_rows))
        _lib.check(rc, "uavqp_repair_rows_from_hits_device")

    # ---- multi-GPU: the ctx owns an RCCL communicator (include/uavqp.h, "Multi-GPU") ----
    @staticmethod
    def comm_unique_id():
        """RCCL rendezvous token (bytes, UAVQP_UNIQUE_ID_BYTES): call on ONE rank, ship it to the others."""
        buf = ctypes.create_string_buffer(_lib.UAVQP_UNIQUE_ID_BYTES)
        _lib.check(_lib.lib().uavqp_comm_unique_id(buf), "uavqp_comm_unique_id")
        return buf.raw

    def comm_create(self, rank, world, unique_id):
        """Collective over all ranks: create the communicator this ctx owns (world = 1 is a valid self test)."""
        assert len(unique_id) == _lib.UAVQP_UNIQUE_ID_BYTES
        buf = ctypes.create_string_buffer(bytes(unique_id), _lib.UAVQP_UNIQUE_ID_BYTES)
        _lib.check(_lib.lib().uavqp_comm_create(self._h, int(rank), int(world), buf), "uavqp_comm_create")
        self.rank, self.world = int(rank), int(world)

    def comm_info(self):
        """(rank, world) of this ctx's communicator as RCCL itself reports them (ncclCommUserRank / ncclCommCount)."""
        rk, wd = ctypes.c_int32(-1), ctypes.c_int32(-1)
        _lib.check(_lib.lib().uavqp_comm_info(self._h, ctypes.byref(rk), ctypes.byref(wd)), "uavqp_comm_info")
        return int(rk.value), int(wd.value)

    def comm_destroy(self):
        _lib.check(_lib.lib().uavqp_comm_destroy(self._h), "uavqp_comm_destroy")

    def allgather_coeffs(self, local, counts, full):
        """RCCL all-gather of float64 device shards on the ctx stream: rank g contributes counts[g] doubles of `local`,
        `full` receives them back to back in rank order (`local` may be the rank's own slice of `full`)."""
        c = (ctypes.c_int64 * len(counts))(*[int(x) for x in counts])
        _lib.check(_lib.lib().uavqp_allgather_coeffs(self._h, _ptr(local), c, _ptr(full)), "uavqp_allgather_coeffs")

    def allgather_status(self, local, counts, full):
        """The same for the int32 status arrays (counts in trajectories)."""
        c = (ctypes.c_int64 * len(counts))(*[int(x) for x in counts])
        _lib.check(_lib.lib().uavqp_allgather_status(self._h, _ptr(local), c, _ptr(full)), "uavqp_allgather_status")

    def capture_begin(self):
        """Start hipGraph capture of everything subsequently enqueued on the ctx stream."""
        _lib.check(_lib.lib().uavqp_capture_begin(self._h), "uavqp_capture_begin")

    def capture_end(self):
        g = ctypes.c_void_p()
        _lib.check(_lib.lib().uavqp_capture_end(self._h, ctypes.byref(g)), "uavqp_capture_end")
        return g

    def graph_launch(self, graph):
        _lib.check(_lib.lib().uavqp_graph_launch(self._h, graph), "uavqp_graph_launch")

    def graph_destroy(self, graph):
        _lib.check(_lib.lib().uavqp_graph_destroy(self._h, graph), "uavqp_graph_destroy")

    def solve_batch_device(self, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc,
                           coeff_out, status_out=None):
        """All array arguments are device buffers (torch CUDA tensors or raw integer addresses). Asynchronous."""
        rc = _lib.lib().uavqp_solve_batch_device(self._h, r, n_traj, uniform_segments, max_segments, _ptr(seg_offsets),
                                                 _ptr(waypoints), _ptr(times), _ptr(bc), _ptr(coeff_out), _ptr(status_out))
        _lib.check(rc, "uavqp_solve_batch_device")

    def solve_batch_host(self, r, seg_offsets, waypoints, times, bc, uniform_segments=0):
        """numpy in / numpy out (H2D + solve + D2H, synchronous).  Returns (coeff_flat, status)."""
        waypoints = np.ascontiguousarray(waypoints, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert waypoints.size == 3 * (total + n_traj), "waypoints must hold sum(M_b + 1) xyz rows"
        assert bc.size == n_traj * 2 * (r - 1) * 3
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_solve_batch_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so),
                                               _ptr(waypoints), _ptr(times), _ptr(bc), _ptr(coeff), _ptr(status))
        _lib.check(rc, "uavqp_solve_batch_host")
        return coeff, status

    def solve_corridor_batch_host(self, r, seg_offsets, waypoints, times, bc, corr_lo, corr_hi, uniform_segments=0):
        """Corridor-constrained solve, numpy in / numpy out.  Returns (coeff_flat, status, iters)."""
        waypoints = np.ascontiguousarray(waypoints, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        lo = np.ascontiguousarray(corr_lo, dtype=np.float64)
        hi = np.ascontiguousarray(corr_hi, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        assert waypoints.size == 3 * (total + n_traj) == lo.size == hi.size
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        iters = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_solve_corridor_batch_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so),
                                                        _ptr(waypoints), _ptr(times), _ptr(bc), _ptr(lo), _ptr(hi),
                                                        _ptr(coeff), _ptr(status), _ptr(iters))
        _lib.check(rc, "uavqp_solve_corridor_batch_host")
        return coeff, status, iters

    def solve_rows_batch_host(self, r, seg_offsets, waypoints, times, bc, corr_lo, corr_hi, rows_per_segment, row_tau, row_deriv,
                              row_lo, row_hi, uniform_segments=0):
        """Knot boxes (or None, None: waypoint equalities) + general rows, numpy in / numpy out (uavqp_solve_rows_batch_host).
        row_tau / row_deriv [segments][K], row_lo / row_hi [segments][K][3].  Returns (coeff_flat, status, iters)."""
        waypoints = np.ascontiguousarray(waypoints, dtype=np.float64)
        times = np.ascontiguousarray(times, dtype=np.float64)
        bc = np.ascontiguousarray(bc, dtype=np.float64)
        lo = None if corr_lo is None else np.ascontiguousarray(corr_lo, dtype=np.float64)
        hi = None if corr_hi is None else np.ascontiguousarray(corr_hi, dtype=np.float64)
        tau = np.ascontiguousarray(row_tau, dtype=np.float64)
        drv = np.ascontiguousarray(row_deriv, dtype=np.int32)
        rlo = np.ascontiguousarray(row_lo, dtype=np.float64)
        rhi = np.ascontiguousarray(row_hi, dtype=np.float64)
        so, n_traj, total, mmax = _batch_shape(seg_offsets, times, uniform_segments)
        K = int(rows_per_segment)
        assert waypoints.size == 3 * (total + n_traj) and tau.size == total * K == drv.size and rlo.size == 3 * total * K == rhi.size
        coeff = np.zeros(3 * 2 * r * total, dtype=np.float64)
        status = np.zeros(n_traj, dtype=np.int32)
        iters = np.zeros(n_traj, dtype=np.int32)
        rc = _lib.lib().uavqp_solve_rows_batch_host(self._h, r, n_traj, uniform_segments, max(mmax, 1), _ptr(so), _ptr(waypoints), _ptr(times),
                                                    _ptr(bc), _ptr(lo), _ptr(hi), K, _ptr(tau), _ptr(drv), _ptr(rlo), _ptr(rhi),
                                                    _ptr(coeff), _ptr(status), _ptr(iters))
        _lib.check(rc, "uavqp_solve_rows_batch_host")
        return coeff, status, iters

    def solve_axis_host(self, r, pos_1d, bound_vel, bound_acc, time_vec, bound_jerk=None):
        pos = np.ascontiguousarray(pos_1d, dtype=np.float64)
        bv = np.ascontiguousarray(bound_vel, dtype=np.float64)
        ba = np.ascontiguousarray(bound_acc, dtype=np.float64)
        bj = None if bound_jerk is None else np.ascontiguousarray(bound_jerk, dtype=np.float64)
        tv = np.ascontiguousarray(time_vec, dtype=np.float64)
        n_seg = tv.size
        coef = np.zeros(2 * r * max(n_seg, 0), dtype=np.float64)
        st = ctypes.c_int32(0)
        rc = _lib.lib().uavqp_solve_axis_host(self._h, r, n_seg, _ptr(pos), _ptr(bv), _ptr(ba), _ptr(bj), _ptr(tv),
                                              _ptr(coef), ctypes.byref(st))
        return rc, st.value, coef


class MinimumControl:
    """Drop-in mirror of traj_optimization::MinimumControl (reference minimum_control.h:10-48).

    solve() keeps the reference's contract: inputs are not modified, the return value is a bool,
    on failure the previously stored coefficients are kept (minimum_control.cpp:173-184), one axis per
    call, coefficients in ascending powers per segment (minimum_control.cpp:186).  `order` selects
    r = 3 (min-jerk, the reference) or r = 4 (min-snap extension; bound_jerk defaults to zero).
    """

    def __init__(self, order=3, device=0):
        assert order in (3, 4)
        self._r = order
        self._device = device
        self._ctx = None  # created on first solve (the reference builds its OSQP workspace in solve(), too)
        self._coef_1d = np.zeros(0)

    def solve(self, pos_1d, bound_vel, bound_acc, time_vec, bound_jerk=None):
        pos = np.asarray(pos_1d, dtype=np.float64)
        tv = np.asarray(time_vec, dtype=np.float64)
        # reference H8: pos_1d.size() < 2 indexes out of range there; here it is a clean failure
        if pos.ndim != 1 or tv.ndim != 1 or tv.size < 1 or pos.size != tv.size + 1:
            print("solver init failed!")
            return False
        if self._ctx is None:
            self._ctx = Context(self._device)  # raises UavqpError without libuavqp.so / without a GPU
            # the three settings the reference passes to its solver (minimum_control.cpp:160-162)
            self._ctx.set_settings(warm_start=1, eps_prim_inf=1e-3, max_iter=1000)
        rc, st, coef = self._ctx.solve_axis_host(self._r, pos, bound_vel, bound_acc, tv, bound_jerk)
        if rc != _lib.UAVQP_OK:
            print("solver init failed!")
            return False
        if st != _lib.UAVQP_SOLVED:
            print("solver solve failed!")
            return False
        self._coef_1d = coef
        return True

    def reset(self):
        """minimum_control.cpp:194-197: coef_1d_.setZero()."""
        self._coef_1d = np.zeros_like(self._coef_1d)

    def getCoef1d(self):
        """minimum_control.cpp:199-202: returns a copy."""
        return self._coef_1d.copy()


class TrajOptimizer:
    """Batch facade with the north-star method names; all trajectories and axes in one device pass.

    setWaypoints(xyz, wp_offsets)    xyz [sum(M_b+1)][3]; wp_offsets[n_traj+1] (or None + uniform count)
    setTimeAllocation(T)             T [sum M_b]
    setBoundary(bc)                  bc [n_traj][2][r-1][3]; default: all zero (test_minimum_jerk.cpp:59-63)
    setCorridor(lo, hi)              optional boxes [sum(M_b+1)][3] replacing the interior-waypoint equalities
                                     (north-star extension; None, None restores the reference's equality rows)
    setRows(K, tau, deriv, lo, hi)   optional general rows lo <= p^(deriv)(tau T) <= hi per segment, slot and axis (K = 1 or 2 slots;
                                     tau / deriv [sum M_b][K], lo / hi [sum M_b][K][3]; K = 0 removes them) -- the same method as the
                                     C++ facade's (cpp/traj_optimizer.h)
    solve() -> bool                  True iff every trajectory solved (statuses in .status)
    optimizeTime(time_weight, ...)   equality-constrained problems only: minimises cost + time_weight * sum T over the durations
                                     (uavqp_time_optimize_host), stores the optimised allocation (getTimeAllocation) and the
                                     coefficients at it; objective [n_traj][2] (start, result) in .objective.  limits = dict of
                                     uavqp_limit_params fields: the soft velocity / acceleration penalty joins the objective
                                     (uavqp_time_optimize_limits_host), .peak [n_traj][2] = sampled |v| / v_max, |a| / a_max at the result
    getLimitPenalty(**limits)        [n_traj] limit penalty of the stored coefficients at the stored durations
    getClearancePenalty(esdf, ...)   [n_traj] clearance penalty of the stored coefficients against an esdf.EsdfMap built on context()
                                     (also spelled get_clearance_penalty)
    optimizeWaypoints(esdf, ...)     equality-constrained problems only: moves the interior waypoints to minimise smooth_weight * cost +
                                     clearance penalty against an esdf.EsdfMap built on context() (uavqp_waypoint_optimize_host); stores
                                     the optimised waypoints (getWaypoints) and the coefficients at them; .objective as for optimizeTime,
                                     .min_dist / .outside [n_traj] the penalty's diagnostics at the result
    optimizeTrajectory(esdf, ...)    equality-constrained problems only: moves the interior waypoints AND the durations together to
                                     minimise smooth_weight * cost + time_weight * sum T + limit penalty + clearance penalty
                                     (uavqp_spacetime_optimize_host); stores waypoints, durations and coefficients; .objective,
                                     .iterations, .peak, .min_dist, .outside as above
    optimizeTrajectoryLbfgs(esdf, ...)   the same with limited-memory BFGS directions kept on the device (uavqp_spacetime_lbfgs_host)
    optimizeTrajectoryAttitude(esdf, ...)   optimizeTrajectoryLbfgs with the attitude penalty (thrust, tilt, body rate) in the objective
                                     (uavqp_attitude_optimize_host); .attitude_peak [n_traj][4] the sampled peaks at the result
    getAttitudePenalty(...)          [n_traj] attitude penalty of the stored coefficients at the stored durations; fills .attitude_peak
    setMovingObstacles(times, coeff, ...)   obstacle tracks that are not this batch's to move (uavqp_moving_obstacles): their sets, which
                                     set each trajectory avoids, the departures on the common clock
    getMovingPenalty(...)            [n_traj] penalty against those tracks; fills .min_gap and .nearest
    getMovingCertificate(...)        certified gap of every segment to those tracks for EVERY t of its flight (lower / upper bounds, verdict)
    optimizeTrajectoryMoving(esdf, ...)   optimizeTrajectoryAttitude with that penalty in the objective (uavqp_moving_optimize_host;
                                     attitude=None: no attitude term); .min_gap / .nearest at the result
    getEnvelope(depth, box, **limits)  certified bounds over whole segments and the certified / violated / undecided masks per limit
    getFlightPenalty(esdf, ...)      [n_traj] limit + clearance penalty of the stored coefficients in one launch
    setSwarm(group_offsets, start_times)   which trajectories fly together (swarm g = trajectories group_offsets[g] .. group_offsets[g + 1];
                                     None: the whole batch is one swarm) and when each departs on its swarm's clock (None: all at 0)
    getSwarmPenalty(...)             [n_groups] separation penalty between the vehicles of each swarm at the stored coefficients
    getSeparationCertificate(...)    certified separation between the vehicles of each swarm for EVERY t of a clock window (lower / upper
                                     bounds, witness, verdict against d_req): the hard test after optimizeSwarm
    optimizeSwarm(esdf, ...)         optimizeTrajectory with that penalty in the objective and one accept / reject per SWARM; with
                                     start_window > 0 the departures are optimised too (getSwarmStart()); .min_sep per trajectory
    getCostWaypointGradient()        [sum (M_b + 1)][3] gradient of getCost() in the waypoints, both ends of every trajectory included
    backward(grad_coeff)             equality-constrained problems only, after solve(): (grad_times, grad_waypoints, grad_bc) of a loss
                                     with d loss / d getPolyCoeff() = grad_coeff, through the solve
    getCost()                        [n_traj] control cost c' P c of the stored coefficients at the stored durations
    getPolyCoeff()                   flat float64 array, trajectory b at 3*2r*seg_offsets[b], [axis][seg][2r]
    """

    def __init__(self, order=4, device=0):
        assert order in (3, 4)
        self._r = order
        self._device = device
        self._ctx = None
        self._wp = self._T = self._bc = self._so = None
        self._lo = self._hi = None
        self._rows = None
        self._groups = self._start = None
        self._moving = None
        self._coef = np.zeros(0)
        self.status = np.zeros(0, dtype=np.int32)
        self.iterations = np.zeros(0, dtype=np.int32)
        self.objective = np.zeros((0, 2))
        self.peak = np.zeros((0, 2))
        self.attitude_peak = np.zeros((0, 4))
        self.min_gap = np.zeros(0)
        self.nearest = np.zeros(0, dtype=np.int32)
        self.min_dist = np.zeros(0)
        self.outside = np.zeros(0, dtype=np.int32)

    def setWaypoints(self, xyz, wp_offsets=None, n_waypoints=None):
        self._wp = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        if wp_offsets is not None:
            wo = np.asarray(wp_offsets, dtype=np.int64)
            n_traj = wo.size - 1
            self._so = (wo - np.arange(n_traj + 1)).astype(np.int32)  # waypoint offsets -> segment offsets
        else:
            assert n_waypoints is not None and n_waypoints >= 2 and self._wp.shape[0] % n_waypoints == 0
            n_traj = self._wp.shape[0] // n_waypoints
            self._so = (np.arange(n_traj + 1) * (n_waypoints - 1)).astype(np.int32)

    def setTimeAllocation(self, T):
        self._T = np.ascontiguousarray(T, dtype=np.float64).ravel()

    def setBoundary(self, bc):
        self._bc = np.ascontiguousarray(bc, dtype=np.float64)

    def setCorridor(self, lo, hi):
        if lo is None or hi is None:
            self._lo = self._hi = None
            return
        self._lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1, 3)
        self._hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1, 3)

    def setRows(self, rows_per_segment, tau=None, deriv=None, lo=None, hi=None):
        if not rows_per_segment:
            self._rows = None
            return
        K = int(rows_per_segment)
        self._rows = (K, np.ascontiguousarray(tau, dtype=np.float64).reshape(-1, K), np.ascontiguousarray(deriv, dtype=np.int32).reshape(-1, K),
                      np.ascontiguousarray(lo, dtype=np.float64).reshape(-1, K, 3), np.ascontiguousarray(hi, dtype=np.float64).reshape(-1, K, 3))

    def solve(self):
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        if self._lo is not None and (self._lo.shape != self._wp.shape or self._hi.shape != self._wp.shape):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        if self._ctx is None:
            self._ctx = Context(self._device)  # raises UavqpError without libuavqp.so / without a GPU
            # the three settings the reference passes to its solver (minimum_control.cpp:160-162)
            self._ctx.set_settings(warm_start=1, eps_prim_inf=1e-3, max_iter=1000)
        if self._rows is not None:
            K, tau, drv, rlo, rhi = self._rows
            if tau.shape[0] != self._T.size:
                return False
            self._coef, self.status, self.iterations = self._ctx.solve_rows_batch_host(
                self._r, self._so, self._wp, self._T, bc, self._lo, self._hi, K, tau, drv, rlo, rhi)
        elif self._lo is not None:
            self._coef, self.status, self.iterations = self._ctx.solve_corridor_batch_host(
                self._r, self._so, self._wp, self._T, bc, self._lo, self._hi)
        else:
            self._coef, self.status = self._ctx.solve_batch_host(self._r, self._so, self._wp, self._T, bc)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def optimizeTime(self, time_weight=None, limits=None, **params):
        """Optimises the stored time allocation (the reference's equality rows only: a corridor or rows set raises ValueError).
        True iff every trajectory is solved at the optimised durations; getPolyCoeff() is the solve at getTimeAllocation().
        limits: None, or a dict of uavqp_limit_params fields ({} = the defaults) -- the soft limit penalty joins the objective and
        .peak holds the sampled |v| / v_max, |a| / a_max at the result (they may exceed 1: include/uavqp.h)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeTime: corridor and general-rows problems are out of scope (include/uavqp.h)")
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        if self._ctx is None:
            self._ctx = Context(self._device)
            self._ctx.set_settings(warm_start=1, eps_prim_inf=1e-3, max_iter=1000)
        if time_weight is not None:
            params["time_weight"] = float(time_weight)
        if limits is not None:
            self._T, self._coef, self.status, self.objective, self.iterations, self.peak = self._ctx.time_optimize_limits_host(
                self._r, self._so, self._wp, self._T, bc, dict(limits), **params)
            return bool(np.all(self.status == _lib.UAVQP_SOLVED))
        self._T, self._coef, self.status, self.objective, self.iterations = self._ctx.time_optimize_host(
            self._r, self._so, self._wp, self._T, bc, **params)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def optimizeWaypoints(self, esdf, smooth_weight=None, clearance=None, **params):
        """Optimises the stored interior waypoints against the distance field `esdf` (an esdf.EsdfMap on this optimiser's context -- see
        context() --, updated); the reference's equality rows only: a corridor or rows set raises ValueError.  True iff every trajectory
        is solved at the optimised waypoints; getPolyCoeff() is the solve at getWaypoints().  clearance: dict of uavqp_clearance_params
        fields; params: fields of uavqp_waypoint_opt_params that differ from the defaults.  The penalty is soft: .min_dist may end below
        d_safe, and .outside counts the samples that left the map (include/uavqp.h)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeWaypoints: corridor and general-rows problems are out of scope (include/uavqp.h)")
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        ctx = self.context()
        if smooth_weight is not None:
            params["smooth_weight"] = float(smooth_weight)
        self._wp, self._coef, self.status, self.objective, self.iterations, self.min_dist, self.outside = ctx.waypoint_optimize_host(
            self._r, self._so, self._wp, self._T, bc, esdf, clearance=clearance, **params)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def optimizeTrajectory(self, esdf, limits=None, clearance=None, **params):
        """Optimises the stored interior waypoints AND the stored time allocation together (uavqp_spacetime_optimize_host): minimises
        smooth_weight * cost + time_weight * sum T + limit penalty + clearance penalty against the distance field `esdf` (an esdf.EsdfMap
        on this optimiser's context -- see context() --, updated).  The reference's equality rows only: a corridor or rows set raises
        ValueError.  True iff every trajectory is solved at the result; getPolyCoeff() is the solve at getWaypoints() and
        getTimeAllocation().  limits / clearance: dicts of uavqp_limit_params / uavqp_clearance_params fields; params: fields of
        uavqp_spacetime_params that differ from the defaults (an unknown field raises ValueError).  .objective [n_traj][2] (start,
        result), .iterations accepted trials, .peak [n_traj][2], .min_dist, .outside the penalties' diagnostics at the result.  Both
        penalties are soft (include/uavqp.h)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeTrajectory: corridor and general-rows problems are out of scope (include/uavqp.h)")
        Context._spacetime_params(params)   # (an unknown field is refused before anything runs)
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        ctx = self.context()
        (self._wp, self._T, self._coef, self.status, self.objective, self.iterations, self.peak, self.min_dist,
         self.outside) = ctx.spacetime_optimize_host(self._r, self._so, self._wp, self._T, bc, esdf, limits=limits, clearance=clearance, **params)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def optimizeTrajectoryLbfgs(self, esdf, limits=None, clearance=None, **params):
        """optimizeTrajectory with limited-memory BFGS directions (uavqp_spacetime_lbfgs_host): the same objective, bounds and members
        filled, fewer trials to the same objective.  params: fields of uavqp_spacetime_lbfgs_params that differ from the defaults (an
        unknown field raises ValueError)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeTrajectoryLbfgs: corridor and general-rows problems are out of scope (include/uavqp.h)")
        Context._spacetime_lbfgs_params(params)   # (an unknown field is refused before anything runs)
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        ctx = self.context()
        (self._wp, self._T, self._coef, self.status, self.objective, self.iterations, self.peak, self.min_dist,
         self.outside) = ctx.spacetime_lbfgs_host(self._r, self._so, self._wp, self._T, bc, esdf, limits=limits, clearance=clearance, **params)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def optimizeTrajectoryAttitude(self, esdf, limits=None, clearance=None, attitude=None, **params):
        """optimizeTrajectoryLbfgs with the attitude penalty (thrust, tilt, body rate) inside the objective
        (uavqp_attitude_optimize_host): the same bounds and members filled, and .attitude_peak [n_traj][4] = largest and smallest specific
        thrust (m/s^2), largest tilt (rad), largest body rate (rad/s) sampled at the result.  attitude: dict of uavqp_attitude_params
        fields ({} or None: the defaults); params: fields of uavqp_spacetime_lbfgs_params (an unknown field of either raises ValueError).
        The penalty is soft: check .attitude_peak against the limits (include/uavqp.h)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeTrajectoryAttitude: corridor and general-rows problems are out of scope (include/uavqp.h)")
        Context._spacetime_lbfgs_params(params)   # (an unknown field is refused before anything runs)
        Context._attitude_params(attitude or {})
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        ctx = self.context()
        (self._wp, self._T, self._coef, self.status, self.objective, self.iterations, self.peak, self.min_dist, self.outside,
         self.attitude_peak) = ctx.attitude_optimize_host(self._r, self._so, self._wp, self._T, bc, esdf, limits=limits, clearance=clearance,
                                                          attitude=attitude, **params)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def setMovingObstacles(self, times, coeff, seg_offsets=None, uniform_segments=0, start=None, radius=None, set_offsets=None, traj_set=None,
                           traj_start=None):
        """The moving obstacles the trajectories avoid (uavqp_moving_obstacles): tracks in the library's own format and the SAME order as
        this optimiser -- times [sum Mo], coeff in the layout of getCoefficients(), seg_offsets [n_obs + 1] or uniform_segments -- with
        their departures `start` and radii [n_obs] (None: zeros), the sets set_offsets [n_sets + 1] (None: one set, all of them), the set
        each trajectory avoids traj_set [n_traj] (-1: none; None with one set: set 0) and the trajectories' own departures traj_start
        [n_traj] (None: zeros).  times None removes them."""
        if times is None:
            self._moving = None
            return
        self._moving = dict(times=np.array(times, dtype=np.float64).ravel(), coeff=np.array(coeff, dtype=np.float64).ravel(),
                            seg_offsets=None if seg_offsets is None else np.array(seg_offsets, dtype=np.int32).ravel(),
                            uniform_segments=int(uniform_segments),
                            start=None if start is None else np.array(start, dtype=np.float64).ravel(),
                            radius=None if radius is None else np.array(radius, dtype=np.float64).ravel(),
                            set_offsets=None if set_offsets is None else np.array(set_offsets, dtype=np.int32).ravel(),
                            traj_set=None if traj_set is None else np.array(traj_set, dtype=np.int32).ravel(),
                            traj_start=None if traj_start is None else np.array(traj_start, dtype=np.float64).ravel())

    def getMovingPenalty(self, **params):
        """[n_traj] penalty against the obstacles of setMovingObstacles() at the stored coefficients and durations
        (uavqp_moving_penalty_host; after solve() or an optimiser); params: fields of uavqp_moving_params that differ from the defaults.
        .min_gap [n_traj] and .nearest [n_traj] are filled with the smallest sampled gap and the obstacle that attains it."""
        if self._moving is None:
            raise _lib.UavqpError("getMovingPenalty: no obstacles (call setMovingObstacles() first)")
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getMovingPenalty: no solved coefficients (call solve() or an optimiser first)")
        phi, _, _, _, self.min_gap, self.nearest = self._ctx.moving_penalty_host(self._r, self._so, self._T, self._coef, self._moving,
                                                                                  status=self.status, **params)
        return phi

    def getMovingCertificate(self, depth=3, d_req=1.0, downwash=1.0):
        """Certified gap of every segment to the obstacles of setMovingObstacles(), at the stored coefficients and durations, for EVERY t of
        the segment (uavqp_moving_certificate_host; after solve() or an optimiser): the hard test that the sampled .min_gap is not.
        Returns a dict: gap [sum M][2] (lower, upper), where [sum M][4] ({obstacle of lower, leaf of lower, obstacle of upper, witness
        index of upper}), peak [n_traj][2], seg_verdict [sum M], verdict [n_traj] (the int32 words) and, per trajectory, the boolean
        masks certified (>= d_req for ALL t), violated (< d_req at the witness) and undecided (raise depth, or replan)."""
        if self._moving is None:
            raise _lib.UavqpError("getMovingCertificate: no obstacles (call setMovingObstacles() first)")
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getMovingCertificate: no solved coefficients (call solve() or an optimiser first)")
        gap, where, peak, seg_verdict, verdict = self._ctx.moving_certificate_host(
            self._r, self._so, self._T, self._coef, self._moving, status=self.status, depth=depth, d_req=d_req, downwash=downwash)
        c, v = verdict & _lib.UAVQP_MOVING_CERT_CERTIFIED != 0, verdict & _lib.UAVQP_MOVING_CERT_VIOLATED != 0
        return dict(gap=gap, where=where, peak=peak, seg_verdict=seg_verdict, verdict=verdict, certified=c, violated=v,
                    undecided=~c & ~v & (self.status == _lib.UAVQP_SOLVED))

    def optimizeTrajectoryMoving(self, esdf, limits=None, clearance=None, attitude=None, moving=None, **params):
        """optimizeTrajectoryAttitude with the penalty against the obstacles of setMovingObstacles() inside the objective
        (uavqp_moving_optimize_host): the same bounds and members filled, and .min_gap / .nearest at the result.  attitude None: NO
        attitude term ({}: its defaults); moving: dict of uavqp_moving_params fields; params: fields of uavqp_spacetime_lbfgs_params (an
        unknown field of any raises ValueError).  The penalty is soft: check .min_gap (include/uavqp.h)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeTrajectoryMoving: corridor and general-rows problems are out of scope (include/uavqp.h)")
        if self._moving is None:
            raise _lib.UavqpError("optimizeTrajectoryMoving: no obstacles (call setMovingObstacles() first)")
        Context._spacetime_lbfgs_params(params)   # (an unknown field is refused before anything runs)
        Context._moving_params(moving or {})
        if attitude is not None:
            Context._attitude_params(attitude)
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        ctx = self.context()
        (self._wp, self._T, self._coef, self.status, self.objective, self.iterations, self.peak, self.min_dist, self.outside,
         self.attitude_peak, self.min_gap, self.nearest) = ctx.moving_optimize_host(
             self._r, self._so, self._wp, self._T, bc, esdf, self._moving, limits=limits, clearance=clearance, attitude=attitude, moving=moving,
             **params)
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def getAttitudePenalty(self, **params):
        """[n_traj] attitude penalty (thrust, tilt, body rate) of the stored coefficients at the stored durations (after solve() or an
        optimiser); params: fields of uavqp_attitude_params that differ from the defaults.  Trajectories that did not solve carry zero.
        .attitude_peak [n_traj][4] is filled with the sampled peaks."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getAttitudePenalty: no solved coefficients (call solve() or an optimiser first)")
        phi, _, _, self.attitude_peak = self._ctx.attitude_penalty_host(self._r, self._so, self._T, self._coef, status=self.status, **params)
        return phi

    def getEnvelope(self, depth=4, box=None, **limits):
        """Certified bounds of the stored coefficients at the stored durations over WHOLE segments (uavqp_envelope_host; after solve() or
        an optimiser): the acceptance test that needs no sampling density.  limits: v_max, a_max, j_max, f_min, f_max, tilt_max (0 or
        absent: off); box: (lo, hi), each [sum M][3], one box per segment.  Returns a dict: range [sum M][4][3][4], norm [sum M][5][4],
        peak [n_traj][5][4], seg_verdict, verdict (the int32 words) and, per trajectory, the boolean masks certified / violated /
        undecided, each a dict keyed by test name (_lib.ENVELOPE_TESTS); a test that is off is False in all three."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getEnvelope: no solved coefficients (call solve() or an optimiser first)")
        box_lo, box_hi = (None, None) if box is None else box
        rng, norm, peak, seg_verdict, verdict = self._ctx.envelope(self._r, self._so, self._T, self._coef, status=self.status, box_lo=box_lo,
                                                                   box_hi=box_hi, depth=depth, **limits)
        on = {name: bool(limits.get(name, 0.0)) for name in _lib.ENVELOPE_TESTS}
        on["box"] = box is not None
        solved = self.status == _lib.UAVQP_SOLVED
        out = dict(range=rng, norm=norm, peak=peak, seg_verdict=seg_verdict, verdict=verdict, certified={}, violated={}, undecided={})
        for k, name in enumerate(_lib.ENVELOPE_TESTS):
            c, v = (verdict >> (2 * k)) & 1 == 1, (verdict >> (2 * k + 1)) & 1 == 1
            out["certified"][name], out["violated"][name] = c, v
            out["undecided"][name] = ~c & ~v & solved if on[name] else np.zeros_like(c)
        return out

    def getClearanceCertificate(self, esdf, depth=4, d_req=0.5):
        """Certified clearance of the stored coefficients at the stored durations against the distance field `esdf` over WHOLE segments
        (uavqp_clearance_certificate_host; after solve() or an optimiser): what no sampled check gives.  Returns a dict: clear [sum M][2]
        (lower, upper), witness [sum M], peak [n_traj][2], seg_verdict, verdict (the int32 words) and, per trajectory, the boolean masks
        certified (>= d_req for ALL t), violated (< d_req at the witness), undecided and outside (a witness point left the map)."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getClearanceCertificate: no solved coefficients (call solve() or an optimiser first)")
        clear, witness, peak, seg_verdict, verdict = self._ctx.clearance_certificate(self._r, self._so, self._T, self._coef, esdf,
                                                                                     status=self.status, depth=depth, d_req=d_req)
        c, v = verdict & _lib.UAVQP_CLEARANCE_CERTIFIED != 0, verdict & _lib.UAVQP_CLEARANCE_VIOLATED != 0
        return dict(clear=clear, witness=witness, peak=peak, seg_verdict=seg_verdict, verdict=verdict, certified=c, violated=v,
                    undecided=~c & ~v & (self.status == _lib.UAVQP_SOLVED), outside=verdict & _lib.UAVQP_CLEARANCE_OUTSIDE != 0)

    def getFlightPenalty(self, esdf, limits=None, clearance=None):
        """[n_traj] limit penalty + clearance penalty of the stored coefficients at the stored durations against `esdf`, in one launch
        (uavqp_flight_penalty_host).  Trajectories that did not solve carry zero."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getFlightPenalty: no solved coefficients (call solve() first)")
        return self._ctx.flight_penalty_host(self._r, self._so, self._T, self._coef, esdf, status=self.status, limits=limits, clearance=clearance)[0]

    def getWaypoints(self):
        return self._wp.copy()

    def getCostWaypointGradient(self):
        """[sum (M_b + 1)][3] gradient of the control cost of the stored coefficients in the waypoints, all knots of every trajectory
        (after solve() of an equality-constrained problem, optimizeTime() or optimizeWaypoints()).  Trajectories that did not solve carry zeros."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("getCostWaypointGradient: corridor and general-rows problems are out of scope (include/uavqp.h)")
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getCostWaypointGradient: no solved coefficients (call solve() first)")
        return self._ctx.cost_waypoint_gradient_host(self._r, self._so, self._coef, status=self.status)

    def getLimitPenalty(self, **limits):
        """[n_traj] limit penalty of the stored coefficients at the stored durations (after solve() or optimizeTime());
        limits: fields of uavqp_limit_params that differ from the defaults.  Trajectories that did not solve carry zero."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getLimitPenalty: no solved coefficients (call solve() or optimizeTime() first)")
        return self._ctx.limit_penalty_host(self._r, self._so, self._T, self._coef, status=self.status, **limits)[0]

    def getClearancePenalty(self, esdf, **params):
        """[n_traj] clearance penalty of the stored coefficients at the stored durations against the distance field `esdf` (an
        esdf.EsdfMap on this optimiser's context -- see context() --, updated); params: fields of uavqp_clearance_params that differ from
        the defaults.  Trajectories that did not solve carry zero."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getClearancePenalty: no solved coefficients (call solve() or optimizeTime() first)")
        return self._ctx.clearance_penalty_host(self._r, self._so, self._T, self._coef, esdf, status=self.status, **params)[0]

    get_clearance_penalty = getClearancePenalty

    def setSwarm(self, group_offsets=None, start_times=None):
        """Which trajectories fly together: swarm g is the trajectories group_offsets[g] .. group_offsets[g + 1] (None: the whole batch is
        one swarm); start_times [n_traj]: when each departs on its swarm's clock (None: all at 0)."""
        self._groups = None if group_offsets is None else np.ascontiguousarray(group_offsets, dtype=np.int32).ravel()
        self._start = None if start_times is None else np.ascontiguousarray(start_times, dtype=np.float64).ravel()

    def getSwarmPenalty(self, **params):
        """[n_groups] separation penalty between the vehicles of each swarm set with setSwarm(), at the stored coefficients and durations
        (uavqp_swarm_penalty_host); params: fields of uavqp_swarm_params that differ from the defaults.  Vehicles that did not solve are
        left out of every pair."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getSwarmPenalty: no solved coefficients (call solve() or optimizeTime() first)")
        return self._ctx.swarm_penalty_host(self._r, self._so, self._T, self._coef, group_offsets=self._groups, start=self._start,
                                            status=self.status, **params)[0]

    def optimizeSwarm(self, esdf, limits=None, clearance=None, swarm=None, **params):
        """optimizeTrajectory for the swarms set with setSwarm() (uavqp_swarm_optimize_host): the separation penalty between the vehicles
        of each swarm joins the objective and every trial is accepted or rejected per SWARM.  With start_window > 0 the departures of
        setSwarm() are optimised too and the new ones stored (getSwarmStart()).  The reference's equality rows only: a corridor or rows
        set raises ValueError.  True iff every trajectory is solved at the result.  limits / clearance / swarm: dicts of
        uavqp_limit_params / uavqp_clearance_params / uavqp_swarm_params fields; params: fields of uavqp_swarm_opt_params that differ from
        the defaults (an unknown field raises ValueError).  Fills the members optimizeTrajectory fills -- .objective [n_groups][2] and
        .iterations [n_groups] per swarm -- and .min_sep [n_traj].  All penalties are soft (include/uavqp.h)."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("optimizeSwarm: corridor and general-rows problems are out of scope (include/uavqp.h)")
        pp = Context._swarm_opt_params(params)   # (an unknown field is refused before anything runs)
        Context._swarm_params(swarm or {})
        if self._wp is None or self._T is None:
            return False
        n_traj = self._so.size - 1
        if self._T.size != int(self._so[-1]):
            return False
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        start = self._start
        if start is None and pp.start_window > 0.0:
            start = np.zeros(n_traj, dtype=np.float64)
        ctx = self.context()
        (self._wp, self._T, start, self._coef, self.status, self.objective, self.iterations, self.peak, self.min_dist, self.outside,
         self.min_sep) = ctx.swarm_optimize_host(self._r, self._so, self._wp, self._T, bc, esdf, group_offsets=self._groups, start=start,
                                                 limits=limits, clearance=clearance, swarm=swarm, **params)
        self._start = start
        return bool(np.all(self.status == _lib.UAVQP_SOLVED))

    def getSeparationCertificate(self, depth=2, d_req=1.0, **clock):
        """Certified separation between the vehicles of each swarm set with setSwarm(), at the stored coefficients, durations and departures,
        for EVERY t of the clock window (uavqp_separation_certificate_host; after solve() or optimizeSwarm()): the hard test that the
        sampled min_sep is not.  clock: n_cells, clock_start, dt, downwash of uavqp_separation_params that differ from the defaults.  Returns
        a dict: lower, upper [n_traj], where [n_traj][4] ({partner of lower, leaf of lower, partner of upper, witness index of upper}),
        verdict [n_traj], group_verdict [n_groups] (the int32 words) and, per trajectory, the boolean masks certified (>= d_req for ALL t of
        the window), violated (< d_req at the witness), undecided, and moving (still under way at the end of the window)."""
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("getSeparationCertificate: no solved coefficients (call solve() or an optimiser first)")
        lower, upper, where, verdict, group_verdict = self._ctx.separation_certificate(
            self._r, self._so, self._T, self._coef, group_offsets=self._groups, start=self._start, status=self.status, depth=depth, d_req=d_req,
            **clock)
        c, v = verdict & _lib.UAVQP_SEPARATION_CERTIFIED != 0, verdict & _lib.UAVQP_SEPARATION_VIOLATED != 0
        return dict(lower=lower, upper=upper, where=where, verdict=verdict, group_verdict=group_verdict, certified=c, violated=v,
                    undecided=~c & ~v & (self.status == _lib.UAVQP_SOLVED), moving=verdict & _lib.UAVQP_SEPARATION_MOVING != 0)

    def getSwarmStart(self):
        """[n_traj] the departures of setSwarm(), as optimizeSwarm() left them (None: all at 0)."""
        return None if self._start is None else self._start.copy()

    def context(self):
        """The Context this optimiser solves on (created on first use): what an esdf.EsdfMap for getClearancePenalty is built on."""
        if self._ctx is None:
            self._ctx = Context(self._device)
            self._ctx.set_settings(warm_start=1, eps_prim_inf=1e-3, max_iter=1000)
        return self._ctx

    def backward(self, grad_coeff):
        """After solve() of an equality-constrained problem: (grad_times, grad_waypoints, grad_bc) as numpy for grad_coeff = dPhi/dcoeff in
        the layout of getPolyCoeff() (uavqp_solve_backward_host).  Trajectories that did not solve carry zeros."""
        if self._lo is not None or self._rows is not None:
            raise ValueError("backward: corridor and general-rows problems are out of scope (include/uavqp.h)")
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]) or self.status.size != self._so.size - 1:
            raise _lib.UavqpError("backward: no solved coefficients (call solve() first)")
        n_traj = self._so.size - 1
        bc = self._bc if self._bc is not None else np.zeros((n_traj, 2, self._r - 1, 3))
        return self._ctx.solve_backward_host(self._r, self._so, self._wp, self._T, bc, self._coef, grad_coeff, status=self.status)

    def getTimeAllocation(self):
        return self._T.copy()

    def getCost(self):
        """[n_traj] c' P c of the stored coefficients (after solve() or optimizeTime()); computed on the device."""
        import torch
        n_traj = self._so.size - 1
        if self._ctx is None or self._coef.size != 3 * 2 * self._r * int(self._so[-1]):
            raise _lib.UavqpError("getCost: no solved coefficients (call solve() or optimizeTime() first)")
        dev = torch.device("cuda", self._device)
        so = torch.from_numpy(self._so).to(dev)
        tt = torch.from_numpy(self._T).to(dev)
        cf = torch.from_numpy(self._coef).to(dev)
        cost = torch.zeros(n_traj, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self._ctx.cost_time_gradient_device(self._r, n_traj, 0, so, tt, cf, cost=cost)
        self._ctx.synchronize()
        return cost.cpu().numpy()

    def getPolyCoeff(self, traj=None):
        if traj is None:
            return self._coef.copy()
        s0, s1 = int(self._so[traj]), int(self._so[traj + 1])
        nc = 2 * self._r
        return self._coef[3 * nc * s0:3 * nc * s1].reshape(3, s1 - s0, nc).copy()
