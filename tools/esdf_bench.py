"""Device time of the distance-field layer: uavqp_esdf_update_device, uavqp_esdf_query_device and
uavqp_clearance_penalty_device, with uavqp_limit_penalty_device on the same batch as the penalty's yardstick.

    python tools/esdf_bench.py [--blocks 9] [--calls 20] [--warmup 3]

  update   200 x 200 x 50 at 0.2 m and 400 x 200 x 30 at 0.1 m, occupancy rasterised from config 5's pillar cloud (19 320 points at the
           bench's settings; inflation 0.2 m), both laid over the cloud's bounding box.  A map's fields are 17 bytes per voxel, far
           beyond the caches at these sizes, so repeated updates of one map do not run from cache.
  query    10^6 points uniformly in the 200 x 200 x 50 map, rotating over ROT point / output sets whose footprint exceeds L2 + MALL.
  penalty  config 2's batch (4096 x 8 segments, r = 4) solved once, shifted into the map; coefficient and gradient buffers rotate likewise.
Timing: HIP events around `calls` back-to-back launches on the ctx stream, divided by calls; the median over `blocks` such blocks after
`warmup` untimed blocks, with min .. max.  One JSON line per measurement.  Bytes: what the passes must move at the least -- the
occupancy once and six sweeps (read + write) of an int32 field, plus the float64 result -- against what this implementation moves.
Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402
from uav_motion_planning_amd.esdf import EsdfMap  # noqa: E402

ROT = 8


def timed(torch, ctx, fn, blocks, calls, warmup):
    """fn(k) enqueues call number k on torch's current stream (the ctx is bound to it); -> (median, min, max) ms per call"""
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    ms, k = [], 0
    for blk in range(warmup + blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn(k)
            k += 1
        e1.record(stream)
        e1.synchronize()
        if blk >= warmup:
            ms.append(e0.elapsed_time(e1) / calls)
    ctx.set_stream(None)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    cloud = W.pillar_cloud(5, n_pillars=60, resolution=0.2)
    d_cloud = torch.from_numpy(np.ascontiguousarray(cloud)).to(dev)
    lo = cloud.min(axis=0) - 0.5
    results = []
    with U.Context(0) as ctx:
        maps = {}
        for name, dims, res in (("200x200x50_at_0.2m", (200, 200, 50), 0.2), ("400x200x30_at_0.1m", (400, 200, 30), 0.1)):
            m = EsdfMap(ctx, dims, tuple(lo), res)
            m.set_cloud(d_cloud, inflation=0.2)
            ctx.synchronize()
            occupied = int(np.count_nonzero(m.read(sq_pos=False, sq_neg=False, dist=False)["occ"]))
            med, mn, mx = timed(torch, ctx, lambda k: m.update(), args.blocks, args.calls, args.warmup)
            nv = m.n_voxels
            least = nv * (1 + 6 * 2 * 4 + 8)           # occupancy, six read + write sweeps of an int32 field, the float64 result
            moved = nv * (1 + 8) + nv * 16 + nv * (16 + 8)   # z: 1 B in, 8 B out; y: 8 in, 8 out; x: 8 in, 8 + 8 out
            results.append(dict(what="update", grid=name, voxels=nv, occupied=occupied, cloud_points=int(cloud.shape[0]), ms=med, ms_min=mn,
                                ms_max=mx, bytes_least=least, bytes_moved=moved, gbps_moved=moved / med / 1e6))
            maps[name] = m
        m = maps["200x200x50_at_0.2m"]
        hi = lo + np.array(m.dims) * m.resolution
        # query: 10^6 points, ROT sets (24 + 8 + 24 + 1 MB each)
        n_pts = 1_000_000
        rng = np.random.default_rng(1)
        sets = [dict(p=torch.from_numpy(rng.uniform(lo - 0.2, hi + 0.2, size=(n_pts, 3))).to(dev), d=torch.empty(n_pts, dtype=torch.float64, device=dev),
                     g=torch.empty((n_pts, 3), dtype=torch.float64, device=dev), i=torch.empty(n_pts, dtype=torch.uint8, device=dev)) for _ in range(ROT)]
        L = U.lib()

        def query(k):
            s = sets[k % ROT]
            L.uavqp_esdf_query_device(ctx._h, m.handle, n_pts, s["p"].data_ptr(), s["d"].data_ptr(), s["g"].data_ptr(), s["i"].data_ptr())
        med, mn, mx = timed(torch, ctx, query, args.blocks, args.calls, args.warmup)
        inside = int(sets[0]["i"].sum())
        results.append(dict(what="query", grid="200x200x50_at_0.2m", points=n_pts, inside=inside, ms=med, ms_min=mn, ms_max=mx,
                            mpoints_per_s=n_pts / med / 1e3))
        del sets
        # penalty: config 2's batch inside the map, beside the limit penalty on the same batch
        b = W.uniform_batch(2, 4096, 8, 4, time_mode="distance")
        r, n, M = 4, 4096, 8
        wp = np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)
        d_wp, d_T = torch.from_numpy(wp).to(dev), torch.from_numpy(np.ascontiguousarray(b["times"], dtype=np.float64).ravel()).to(dev)
        d_bc = torch.from_numpy(np.ascontiguousarray(b["bc"], dtype=np.float64)).to(dev)
        coeff = torch.zeros(3 * 2 * r * n * M, dtype=torch.float64, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, coeff, status)
        ctx.synchronize()
        rot = 64      # 64 x (1.5 MB coeff + 1.5 MB grad_coeff + ...) ~ 200 MB
        psets = [dict(c=coeff.clone(), g=torch.empty_like(coeff), gt=torch.empty_like(d_T), p=torch.empty(n, dtype=torch.float64, device=dev),
                      md=torch.empty(n, dtype=torch.float64, device=dev), o=torch.empty(n, dtype=torch.int32, device=dev),
                      pk=torch.empty((n, 2), dtype=torch.float64, device=dev)) for _ in range(rot)]

        def clearance(k):
            s = psets[k % rot]
            ctx.clearance_penalty_device(r, n, M, None, d_T, s["c"], m, status=status, penalty=s["p"], grad_coeff=s["g"], grad_times=s["gt"],
                                         min_dist=s["md"], outside=s["o"], d_safe=1.0)

        def limits(k):
            s = psets[k % rot]
            ctx.limit_penalty_device(r, n, M, None, d_T, s["c"], status=status, penalty=s["p"], grad_coeff=s["g"], grad_times=s["gt"], peak=s["pk"],
                                     v_max=1.5, a_max=2.0)
        c_med, c_mn, c_mx = timed(torch, ctx, clearance, args.blocks, args.calls, args.warmup)
        penalised = int((psets[0]["p"] > 0).sum())
        outside = int((psets[0]["o"] > 0).sum())
        l_med, l_mn, l_mx = timed(torch, ctx, limits, args.blocks, args.calls, args.warmup)
        results.append(dict(what="penalty", batch="config2_4096x8_r4", samples_per_seg=8, penalised=penalised, leaving_the_map=outside,
                            clearance_ms=c_med, clearance_ms_min=c_mn, clearance_ms_max=c_mx, limit_ms=l_med, limit_ms_min=l_mn, limit_ms_max=l_mx,
                            limit_penalised=int((psets[0]["p"] > 0).sum()), ratio=c_med / l_med))
        for mm in maps.values():
            mm.close()
    for res in results:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
