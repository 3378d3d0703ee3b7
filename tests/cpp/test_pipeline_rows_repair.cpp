// The corridor pipeline's rows repair from C++: TrajOptimizer::solvePipeline(..., PipelineRepair::Rows) on a small ragged batch of
// straight paths, each crossing a thin pillar in the middle of one segment (the knots keep their distance from it, so only the final
// check sees the collision).  Checked: the call succeeds, every trajectory is SOLVED, rows were placed, every kept row holds on the
// returned polynomials, the knot boxes are those of the box repair's call without repair rounds.  Built and run by
// tests/test_gpu_repair_rows.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "traj_optimizer.h"

int main() {
    const int r = 4, n = 3;
    const int segs_of[n] = {4, 5, 3};
    std::vector<int32_t> wp_off(n + 1, 0);
    for (int b = 0; b < n; ++b) wp_off[b + 1] = wp_off[b] + segs_of[b] + 1;
    const int rows = wp_off[n], segs = rows - n;
    std::vector<double> xyz(3 * rows), T(segs, 1.0), bc(static_cast<size_t>(n) * 2 * (r - 1) * 3, 0.0), cloud;
    for (int b = 0; b < n; ++b) {
        const double y = 6.0 * b;
        for (int i = wp_off[b]; i < wp_off[b + 1]; ++i) {
            xyz[3 * i] = 1.5 * (i - wp_off[b]);
            xyz[3 * i + 1] = y;
            xyz[3 * i + 2] = 1.0;
        }
        // a pillar 5 cm beside the path, half way along segment 1
        for (int k = 0; k <= 20; ++k) {
            cloud.push_back(2.25);
            cloud.push_back(y + 0.05);
            cloud.push_back(0.1 * k);
        }
    }
    const int n_obs = static_cast<int>(cloud.size() / 3);
    traj_optimization::TrajOptimizer boxes(r), rowsopt(r);
    for (auto* o : {&boxes, &rowsopt}) {
        o->setWaypoints(xyz.data(), wp_off.data(), n);
        o->setTimeAllocation(T.data());
        o->setBoundary(bc.data());
    }
    uavqp_pipeline_params pp;
    uavqp_default_pipeline_params(&pp);
    pp.repair_rounds = 0;
    if (!boxes.solvePipeline(cloud.data(), n_obs, &pp)) { std::printf("box pipeline failed\n"); return 2; }
    pp.repair_rounds = 2;
    if (!rowsopt.solvePipeline(cloud.data(), n_obs, &pp, traj_optimization::PipelineRepair::Rows)) { std::printf("rows pipeline failed\n"); return 3; }
    const uavqp_pipeline_result& res = rowsopt.pipelineResult();
    std::printf("colliding before %d, after %d, repairs %d, rows kept %d\n", res.colliding_before_repair, res.colliding_after, res.repairs,
                rowsopt.repairRows());
    int bad = 0;
    if (res.colliding_before_repair != n || rowsopt.repairRows() < 1 || res.repairs < 1) ++bad;
    if (rowsopt.repairRowDeriv().size() != static_cast<size_t>(2 * segs) || rowsopt.repairRowLo().size() != static_cast<size_t>(6 * segs)) ++bad;
    for (size_t i = 0; i < boxes.corridorLo().size(); ++i)
        if (boxes.corridorLo()[i] != rowsopt.corridorLo()[i] || boxes.corridorHi()[i] != rowsopt.corridorHi()[i]) ++bad;
    int kept = 0;
    for (int b = 0; b < n; ++b) {
        if (rowsopt.status()[b] != UAVQP_SOLVED) ++bad;
        for (int i = 0; i < segs_of[b]; ++i) {
            const int s = wp_off[b] - b + i;
            for (int j = 0; j < 2; ++j) {
                if (rowsopt.repairRowDeriv()[2 * s + j] < 0) continue;
                ++kept;
                const double t = rowsopt.repairRowTau()[2 * s + j] * rowsopt.timeAllocation()[s];
                for (int a = 0; a < 3; ++a) {
                    const double* c = rowsopt.getPolyCoeff(b, a) + 2 * r * i;
                    double p = 0.0;
                    for (int q = 2 * r - 1; q >= 0; --q) p = p * t + c[q];
                    const double lo = rowsopt.repairRowLo()[3 * (2 * s + j) + a], hi = rowsopt.repairRowHi()[3 * (2 * s + j) + a];
                    if (!(p >= lo - 1e-9 && p <= hi + 1e-9)) {
                        std::printf("row (%d, %d, %d) axis %d: %.12f not in [%.12f, %.12f]\n", b, i, j, a, p, lo, hi);
                        ++bad;
                    }
                }
            }
        }
    }
    if (kept != rowsopt.repairRows()) ++bad;
    if (bad) { std::printf("FAILED (%d)\n", bad); return 1; }
    std::printf("OK\n");
    return 0;
}
