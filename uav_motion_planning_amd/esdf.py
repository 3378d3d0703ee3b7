"""EsdfMap -- a signed Euclidean distance field of an occupancy grid on the device (uavqp_esdf_* of include/uavqp.h).

Replaces the three calls a planner makes on the reference's plan_env/SDFMap: cloudCallback (set_cloud), updateESDF3d (update) and
getDistWithGradTrilinear (query).  The map owns its device buffers; every call but the numpy forms is asynchronous on the ctx stream.

    m = EsdfMap(ctx, dims=(200, 200, 50), origin=(-10.0, -10.0, 0.0), resolution=0.1)
    m.set_cloud(points, inflation=0.2)      # numpy [n][3] or a float64 device tensor
    m.update()
    dist, grad, inside = m.query(pts)       # numpy in -> numpy out; device tensor in -> device tensors out

torch is used only for device memory.  No CPU path: without libuavqp.so or a GPU the constructor raises.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .traj_optimizer import _ptr


class EsdfMap:
    def __init__(self, ctx, dims, origin, resolution, max_dist=10000.0):
        """max_dist: the distance reported where the grid holds no obstacle at all (10000 is the reference's buffer fill)."""
        self._ctx = ctx
        self._h = ctypes.c_void_p()
        self.dims = tuple(int(d) for d in dims)
        self.origin = tuple(float(o) for o in origin)
        self.resolution = float(resolution)
        self.max_dist = float(max_dist)
        if len(self.dims) != 3 or len(self.origin) != 3:
            raise ValueError("EsdfMap: dims and origin have three entries")
        d3 = (ctypes.c_int32 * 3)(*self.dims)
        o3 = (ctypes.c_double * 3)(*self.origin)
        rc = _lib.lib().uavqp_esdf_create(ctx._h, ctypes.byref(d3), ctypes.byref(o3), self.resolution, self.max_dist, ctypes.byref(self._h))
        _lib.check(rc, "uavqp_esdf_create")

    @property
    def handle(self):
        """The uavqp_esdf* for the C-ABI entries (Context.clearance_penalty_device)."""
        return self._h

    @property
    def n_voxels(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().uavqp_esdf_destroy(self._ctx._h, self._h)
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

    def _torch(self):
        import torch
        return torch, torch.device("cuda", self._ctx.device)

    def _to_device(self, x, dtype):
        """numpy -> a device tensor of `dtype` (kept alive by the caller until the stream has run); a device tensor passes through"""
        torch, dev = self._torch()
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(dev)
        return x

    def set_occupancy(self, occ):
        """occ: [nx][ny][nz] bytes, 0 free / non-zero occupied -- numpy (synchronous) or a uint8 device tensor (asynchronous)."""
        host = isinstance(occ, np.ndarray) or not hasattr(occ, "data_ptr")
        d = self._to_device(occ, np.uint8)
        if d.numel() != self.n_voxels:
            raise ValueError("set_occupancy: occ must hold one byte per voxel")
        _lib.check(_lib.lib().uavqp_esdf_set_occupancy_device(self._ctx._h, self._h, _ptr(d)), "uavqp_esdf_set_occupancy_device")
        if host:
            self._ctx.synchronize()

    def inflation_steps(self, inflation):
        """The reference's mapping (cloudCallback): ceil(inflation / resolution) voxel steps in x and y, 1 in z."""
        return int(math.ceil(float(inflation) / self.resolution)), 1

    def set_cloud(self, points, inflation=0.0, inflate_xy=None, inflate_z=None, clear_first=True):
        """Marks the inflated cloud.  inflation in metres is mapped the reference's way (inflation_steps); inflate_xy / inflate_z give the
        voxel steps directly.  points: [n][3] numpy (synchronous) or float64 device tensor (asynchronous)."""
        ixy, iz = self.inflation_steps(inflation)
        ixy = ixy if inflate_xy is None else int(inflate_xy)
        iz = iz if inflate_z is None else int(inflate_z)
        host = isinstance(points, np.ndarray) or not hasattr(points, "data_ptr")
        d = self._to_device(points, np.float64)
        if d.numel() % 3:
            raise ValueError("set_cloud: points must be [n][3]")
        rc = _lib.lib().uavqp_esdf_rasterize_cloud_device(self._ctx._h, self._h, _ptr(d) if d.numel() else None, d.numel() // 3, ixy, iz,
                                                          1 if clear_first else 0)
        _lib.check(rc, "uavqp_esdf_rasterize_cloud_device")
        if host:
            self._ctx.synchronize()

    def update(self):
        """Occupancy -> sq_pos, sq_neg, dist (asynchronous)."""
        _lib.check(_lib.lib().uavqp_esdf_update_device(self._ctx._h, self._h), "uavqp_esdf_update_device")

    def read(self, occ=True, sq_pos=True, sq_neg=True, dist=True):
        """-> dict of numpy arrays [nx][ny][nz] of the requested fields (synchronous)."""
        torch, dev = self._torch()
        want = (("occ", occ, torch.uint8), ("sq_pos", sq_pos, torch.int32), ("sq_neg", sq_neg, torch.int32), ("dist", dist, torch.float64))
        bufs = {k: torch.empty(self.n_voxels, dtype=t, device=dev) for k, w, t in want if w}
        torch.cuda.synchronize(dev)
        rc = _lib.lib().uavqp_esdf_read_device(self._ctx._h, self._h, _ptr(bufs.get("occ")), _ptr(bufs.get("sq_pos")), _ptr(bufs.get("sq_neg")),
                                               _ptr(bufs.get("dist")))
        _lib.check(rc, "uavqp_esdf_read_device")
        self._ctx.synchronize()
        return {k: v.cpu().numpy().reshape(self.dims) for k, v in bufs.items()}

    def query(self, pts):
        """(dist [n], grad [n][3], inside [n] uint8) at pts [n][3].  numpy in: uavqp_esdf_query_host, numpy out.  Device tensor in:
        uavqp_esdf_query_device, device tensors out (asynchronous)."""
        if isinstance(pts, np.ndarray) or not hasattr(pts, "data_ptr"):
            p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
            n = p.shape[0]
            dist, grad, inside = np.zeros(n), np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
            rc = _lib.lib().uavqp_esdf_query_host(self._ctx._h, self._h, n, _ptr(p), _ptr(dist), _ptr(grad), _ptr(inside))
            _lib.check(rc, "uavqp_esdf_query_host")
            return dist, grad, inside
        torch, _ = self._torch()
        if pts.dtype != torch.float64 or not pts.is_contiguous() or pts.numel() % 3:
            raise ValueError("query: pts must be a contiguous float64 tensor [n][3]")
        n = pts.numel() // 3
        dist = torch.empty(n, dtype=torch.float64, device=pts.device)
        grad = torch.empty((n, 3), dtype=torch.float64, device=pts.device)
        inside = torch.empty(n, dtype=torch.uint8, device=pts.device)
        rc = _lib.lib().uavqp_esdf_query_device(self._ctx._h, self._h, n, _ptr(pts), _ptr(dist), _ptr(grad), _ptr(inside))
        _lib.check(rc, "uavqp_esdf_query_device")
        return dist, grad, inside
