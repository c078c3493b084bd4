// The adapter's evaluateVarianceRobust, evaluateVarianceRobustPairs, evaluateVarianceRobustPoseDeltas and
// evaluateVarianceRobustTransforms, non-Eigen branch: compiled and linked with -Wall -Werror by tests/test_variance_robust_abi.py.
// Without arguments the driver only checks what needs no device and exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>
#include <limits>

namespace {

// a low-dose caller with an instrument in the field: one pass without the loss for the scale, then the value, an index list, a
// batch of poses, a population of transforms
double variance_robust(EpipolarConsistency::MetricRadonIntermediate& ecc, float floor, int n_source, int n_target)
{
    typedef EpipolarConsistency::MetricRadonIntermediate M;
    double mean_weight = 0.0, inlier_mass = 0.0;
    std::vector<float> pairs;
    double v = ecc.evaluateVarianceRobust(ECC_LOSS_TRUNCATED, std::numeric_limits<float>::infinity(), floor, 0x0, 0x0, &pairs);
    const float delta = (float)M::varianceRobustScale(pairs, 2.0);
    v += ecc.evaluateVarianceRobust(ECC_LOSS_TRUNCATED, delta, floor);
    v += ecc.evaluateVarianceRobust(ECC_LOSS_HUBER, delta, floor, &mean_weight);
    v += ecc.evaluateVarianceRobust(ECC_LOSS_GEMAN_MCCLURE, delta, floor, &mean_weight, &inlier_mass, &pairs);
    std::vector<int> idx(4);
    idx[1] = idx[3] = 1;
    v += ecc.evaluateVarianceRobustPairs(idx, ECC_LOSS_TRUNCATED, delta, floor);
    v += ecc.evaluateVarianceRobustPairs(idx, ECC_LOSS_TRUNCATED, delta, floor, &mean_weight, &inlier_mass, &pairs);
    std::vector<std::vector<int> > moved_views(2, std::vector<int>(1, 0));
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(2, std::vector<Geometry::ProjectionMatrix>(1));
    std::vector<double> values, mean_weights, inlier_masses;
    ecc.evaluateVarianceRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_TRUNCATED, delta, floor, values);
    ecc.evaluateVarianceRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_TRUNCATED, delta, floor, values, &mean_weights, &inlier_masses);
    v += values[0] + mean_weights[1] + inlier_masses[1];
    std::vector<Geometry::RP3Homography> Ts(3);
    Ts[1](0, 3) = 6.0;   // a translation
    std::vector<float> terms(4 * Ts.size() * (size_t)n_source * (size_t)n_target);
    ecc.evaluateVarianceRobustTransforms(n_source, Ts, ECC_LOSS_TRUNCATED, delta, floor, values);
    ecc.evaluateVarianceRobustTransforms(n_source, Ts, ECC_LOSS_TRUNCATED, delta, floor, values, &mean_weights);
    ecc.evaluateVarianceRobustTransforms(n_source, Ts, ECC_LOSS_TRUNCATED, delta, floor, values, &mean_weights, &inlier_masses, terms.data());
    ecc.evaluateVarianceRobustTransforms(n_source, Ts, ECC_LOSS_TRUNCATED, delta, floor, values, 0x0, 0x0, terms.data());
    return v + values[2] + mean_weights[1] + inlier_masses[0] + terms[0] + mean_weight + inlier_mass + (pairs.empty() ? 0.0 : pairs[0] + pairs[3]);
}

}  // namespace

int main(int argc, char** argv)
{
    typedef EpipolarConsistency::MetricRadonIntermediate M;
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    Geometry::RP3Homography I;
    double value = -1.0, mean_weight = -1.0, inlier_mass = -1.0;
    float pairs[4] = {-1.f, -1.f, -1.f, -1.f};
    if (ecc_metric_evaluate_variance_robust(0x0, ECC_LOSS_TRUNCATED, 2.f, 1.f, &value, &mean_weight, &inlier_mass, pairs) != ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_evaluate_variance_robust(0x0, 9, 0.f, 0.f, 0x0, 0x0, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_variance_robust_transforms(0x0, 1, 1, I.data(), ECC_LOSS_HUBER, 2.f, 1.f, &value, &mean_weight, &inlier_mass, pairs) !=
        ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (value != -1.0 || mean_weight != -1.0 || inlier_mass != -1.0 || pairs[0] != -1.f || pairs[3] != -1.f) return 1;
    // the host helper through the adapter: r = 4, 0, 9, 16 -- the live roots are 2, 3, 4
    std::vector<float> rows(16, 1.f);
    rows[3] = 4.f, rows[7] = 0.f, rows[11] = 9.f, rows[15] = 16.f;
    if (M::varianceRobustScale(rows, 2.0) != 6.0) return 1;
    if (M::varianceRobustScale(std::vector<float>(rows.begin(), rows.begin() + 12)) != 2.5) return 1;
    if (M::varianceRobustScale(std::vector<float>()) != 0.0) return 1;
    bool refused = false;
    try {
        M::varianceRobustScale(std::vector<float>(3, 1.f));
    } catch (const std::exception&) {
        refused = true;
    }
    if (!refused) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&variance_robust;
    return 0;
}
