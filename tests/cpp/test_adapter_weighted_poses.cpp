// The adapter's evaluateWeightedPairs and evaluateWeightedPoseDeltas, non-Eigen branch: compiled and linked with -Wall -Werror by
// tests/test_weighted_poses_abi.py.  Without arguments the driver only checks what needs no device and exits with 2; the functions
// below are there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

double weighted_pairs(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<int> idx;
    for (int q = 0; q < 3; ++q) {
        const int t[4] = {q, q + 1, q, q + 1};
        idx.insert(idx.end(), t, t + 4);
    }
    double coverage = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateWeightedPairs(idx);
    v += ecc.evaluateWeightedPairs(idx, &coverage);
    v += ecc.evaluateWeightedPairs(idx, &coverage, &terms);
    v += ecc.evaluateWeightedPairs(idx, 0x0, &terms);
    return v + coverage + (terms.empty() ? 0.0 : terms[0] + terms[1]);
}

double weighted_poses(EpipolarConsistency::MetricRadonIntermediate& ecc, const std::vector<Geometry::ProjectionMatrix>& Ps)
{
    std::vector<std::vector<int> > moved(2);
    std::vector<std::vector<Geometry::ProjectionMatrix> > mats(2);
    moved[0].push_back(1);
    mats[0].push_back(Ps[1]);
    std::vector<double> values, coverages;
    ecc.evaluateWeightedPoseDeltas(moved, mats, values);
    ecc.evaluateWeightedPoseDeltas(moved, mats, values, &coverages);
    return values[0] + values[1] + coverages[0];
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    const int32_t idx[4] = {0, 1, 0, 1}, off[2] = {0, 0};
    double value = -1.0, coverage = -1.0;
    float terms[2] = {-1.f, -1.f};
    if (ecc_metric_evaluate_weighted_pairs(0x0, idx, 1, &value, &coverage, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_weighted_pose_deltas(0x0, 1, off, 0x0, 0x0, &value, &coverage) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || coverage != -1.0 || terms[0] != -1.f || terms[1] != -1.f) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&weighted_pairs;
    (void)&weighted_poses;
    return 0;
}
