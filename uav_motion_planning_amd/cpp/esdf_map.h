// uavqp::EsdfMap -- the distance-field calls of the reference's plan_env/SDFMap over the C ABI (include/uavqp.h: uavqp_esdf_*), with the
// reference's method names where they exist: setOccupied(pos), updateESDF3d(), getDistance(pos), getDistWithGradTrilinear(pos, grad);
// plus setCloud (cloudCallback's marking, the inflation mapped to voxel steps the reference's way) and batch forms of the two queries.
// Header-only, no Eigen: positions are double[3].  The field lives on the device; the map keeps a host copy of the occupancy bytes
// (setOccupied edits it, updateESDF3d uploads it when it changed) and fetches the distances once per update for getDistance.
// Needs the HIP runtime API for those copies, like the sharded entry of traj_optimizer.h.
#ifndef UAVQP_ESDF_MAP_H_
#define UAVQP_ESDF_MAP_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/uavqp.h"

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

namespace uavqp {

class EsdfMap {
  public:
    // ctx is borrowed (TrajOptimizer::context(), or one of the caller's) and must outlive the map.  max_dist: the distance reported where
    // the grid holds no obstacle at all (10000 is the reference's buffer fill).
    EsdfMap(uavqp_ctx* ctx, const int32_t dims[3], const double origin[3], double resolution, double max_dist = 10000.0)
        : ctx_(ctx), res_(resolution) {
        for (int k = 0; k < 3; ++k) { dims_[k] = dims[k]; origin_[k] = origin[k]; }
        if (uavqp_esdf_create(ctx, dims, origin, resolution, max_dist, &map_) != UAVQP_OK) { map_ = nullptr; return; }
        occ_.assign(static_cast<size_t>(dims[0]) * dims[1] * dims[2], 0);
    }
    ~EsdfMap() {
        if (map_) uavqp_esdf_destroy(ctx_, map_);
        if (d_tmp_) (void)hipFree(d_tmp_);
    }
    EsdfMap(const EsdfMap&) = delete;
    EsdfMap& operator=(const EsdfMap&) = delete;

    bool valid() const { return map_ != nullptr; }
    const uavqp_esdf* handle() const { return map_; }

    bool isInMap(const double pos[3]) const {
        for (int k = 0; k < 3; ++k)
            if (pos[k] < origin_[k] + 1e-4 || pos[k] > origin_[k] + dims_[k] * res_ - 1e-4) return false;
        return true;
    }
    void posToIndex(const double pos[3], int id[3]) const {
        for (int k = 0; k < 3; ++k) id[k] = static_cast<int>(std::floor((pos[k] - origin_[k]) * (1.0 / res_)));
    }
    // SDFMap::setOccupied: marks the voxel that holds pos (nothing outside the map); takes effect at the next updateESDF3d().
    void setOccupied(const double pos[3]) {
        if (!map_ || !isInMap(pos)) return;
        int id[3];
        posToIndex(pos, id);
        for (int k = 0; k < 3; ++k) id[k] = std::max(0, std::min(id[k], dims_[k] - 1));
        occ_[address(id)] = 1;
        host_dirty_ = true;
    }
    // cloudCallback's marking without its camera window: every point inflated by ceil(inflation / resolution) voxel steps in x and y and
    // one in z.  xyz: n points on the HOST.  clear_first = false keeps what is already marked.
    bool setCloud(const double* xyz, int n, double inflation, bool clear_first = true) {
        if (!map_ || n < 0 || (n > 0 && !xyz)) return false;
        if (!clear_first && !flush()) return false;
        const size_t bytes = sizeof(double) * 3 * static_cast<size_t>(n);
        if (!scratch(std::max(bytes, occ_.size()))) return false;
        if (n > 0 && hipMemcpy(d_tmp_, xyz, bytes, hipMemcpyHostToDevice) != hipSuccess) return false;
        const int step = static_cast<int>(std::ceil(inflation / res_));
        if (uavqp_esdf_rasterize_cloud_device(ctx_, map_, static_cast<const double*>(d_tmp_), n, step, 1, clear_first ? 1 : 0) != UAVQP_OK) return false;
        // the host copy follows the device
        if (uavqp_synchronize(ctx_) != UAVQP_OK) return false;
        if (uavqp_esdf_read_device(ctx_, map_, static_cast<uint8_t*>(d_tmp_), nullptr, nullptr, nullptr) != UAVQP_OK) return false;
        if (uavqp_synchronize(ctx_) != UAVQP_OK) return false;
        if (hipMemcpy(occ_.data(), d_tmp_, occ_.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
        host_dirty_ = false;
        return true;
    }
    const std::vector<uint8_t>& occupancy() const { return occ_; }

    // SDFMap::updateESDF3d over the whole grid.
    bool updateESDF3d() {
        if (!map_ || !flush()) return false;
        dist_.clear();
        updated_ = uavqp_esdf_update_device(ctx_, map_) == UAVQP_OK;
        return updated_;
    }

    // SDFMap::getDistWithGradTrilinear; outside the map 0 with a zero gradient.  NaN before the first update.
    double getDistWithGradTrilinear(const double pos[3], double grad[3]) {
        double d = std::nan("");
        if (!getDistWithGradTrilinear(pos, 1, &d, grad, nullptr)) grad[0] = grad[1] = grad[2] = d = std::nan("");
        return d;
    }
    // batch form: pos [n][3] on the host -> dist [n], grad [n][3], inside [n] (each may be null)
    bool getDistWithGradTrilinear(const double* pos, int n, double* dist, double* grad, uint8_t* inside) {
        return map_ && updated_ && uavqp_esdf_query_host(ctx_, map_, n, pos, dist, grad, inside) == UAVQP_OK;
    }
    // SDFMap::getDistance: the value of the voxel that holds pos, the index clamped into the grid (boundIndex).  NaN before the first update.
    double getDistance(const double pos[3]) {
        double d = std::nan("");
        getDistance(pos, 1, &d);
        return d;
    }
    bool getDistance(const double* pos, int n, double* dist) {
        if (!fetch()) return false;
        for (int i = 0; i < n; ++i) {
            int id[3];
            posToIndex(pos + 3 * i, id);
            for (int k = 0; k < 3; ++k) id[k] = std::max(0, std::min(id[k], dims_[k] - 1));
            dist[i] = dist_[address(id)];
        }
        return true;
    }

  private:
    size_t address(const int id[3]) const { return (static_cast<size_t>(id[0]) * dims_[1] + id[1]) * dims_[2] + id[2]; }
    bool scratch(size_t bytes) {
        if (bytes <= tmp_bytes_) return true;
        if (uavqp_synchronize(ctx_) != UAVQP_OK) return false;
        if (d_tmp_) (void)hipFree(d_tmp_);
        d_tmp_ = nullptr;
        tmp_bytes_ = 0;
        if (hipMalloc(&d_tmp_, bytes) != hipSuccess) return false;
        tmp_bytes_ = bytes;
        return true;
    }
    // host occupancy -> device, if setOccupied changed it
    bool flush() {
        if (!host_dirty_) return true;
        if (!scratch(occ_.size())) return false;
        if (uavqp_synchronize(ctx_) != UAVQP_OK) return false;
        if (hipMemcpy(d_tmp_, occ_.data(), occ_.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
        if (uavqp_esdf_set_occupancy_device(ctx_, map_, static_cast<const uint8_t*>(d_tmp_)) != UAVQP_OK) return false;
        if (uavqp_synchronize(ctx_) != UAVQP_OK) return false;
        host_dirty_ = false;
        return true;
    }
    // distances -> host, once per update
    bool fetch() {
        if (!map_ || !updated_) return false;
        if (!dist_.empty()) return true;
        const size_t n = occ_.size();
        if (!scratch(sizeof(double) * n)) return false;
        if (uavqp_esdf_read_device(ctx_, map_, nullptr, nullptr, nullptr, static_cast<double*>(d_tmp_)) != UAVQP_OK) return false;
        if (uavqp_synchronize(ctx_) != UAVQP_OK) return false;
        dist_.resize(n);
        if (hipMemcpy(dist_.data(), d_tmp_, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) { dist_.clear(); return false; }
        return true;
    }

    uavqp_ctx* ctx_;
    uavqp_esdf* map_ = nullptr;
    int dims_[3];
    double origin_[3], res_;
    std::vector<uint8_t> occ_;
    std::vector<double> dist_;
    void* d_tmp_ = nullptr;
    size_t tmp_bytes_ = 0;
    bool host_dirty_ = false, updated_ = false;
};

}  // namespace uavqp
#endif
