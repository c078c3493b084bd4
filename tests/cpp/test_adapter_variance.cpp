// The adapter's evaluateVariance, evaluateVariancePairs, evaluateVariancePoseDeltas and evaluateVarianceTransforms, non-Eigen
// branch: compiled and linked with -Wall -Werror by tests/test_variance_abi.py.  Without arguments the driver only checks what needs
// no device and exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// a low-dose caller: the floor from the fields, the value, an index list, a batch of poses, a population of transforms
double variance(EpipolarConsistency::MetricRadonIntermediate& ecc, const std::vector<float>& fields, int n_source, int n_target)
{
    const float floor = EpipolarConsistency::MetricRadonIntermediate::varianceFloor(fields);
    double mean_weight = 0.0;
    std::vector<float> pairs;
    double v = ecc.evaluateVariance(floor);
    v += ecc.evaluateVariance(floor, &mean_weight);
    v += ecc.evaluateVariance(floor, &mean_weight, &pairs);
    v += ecc.evaluateVariance(floor, 0x0, &pairs);
    std::vector<int> idx(4);
    idx[1] = idx[3] = 1;
    v += ecc.evaluateVariancePairs(idx, floor);
    v += ecc.evaluateVariancePairs(idx, floor, &mean_weight, &pairs);
    std::vector<std::vector<int> > moved_views(2, std::vector<int>(1, 0));
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(2, std::vector<Geometry::ProjectionMatrix>(1));
    std::vector<double> values, mean_weights;
    ecc.evaluateVariancePoseDeltas(moved_views, moved_Ps, floor, values);
    ecc.evaluateVariancePoseDeltas(moved_views, moved_Ps, floor, values, &mean_weights);
    v += values[0] + mean_weights[1];
    std::vector<Geometry::RP3Homography> Ts(3);
    Ts[1](0, 3) = 6.0;   // a translation
    std::vector<float> terms(2 * Ts.size() * (size_t)n_source * (size_t)n_target);
    ecc.evaluateVarianceTransforms(n_source, Ts, floor, values);
    ecc.evaluateVarianceTransforms(n_source, Ts, floor, values, &mean_weights);
    ecc.evaluateVarianceTransforms(n_source, Ts, floor, values, &mean_weights, terms.data());
    ecc.evaluateVarianceTransforms(n_source, Ts, floor, values, 0x0, terms.data());
    return v + values[2] + mean_weights[1] + terms[0] + mean_weight + (pairs.empty() ? 0.0 : pairs[0] + pairs[1]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    Geometry::RP3Homography I;
    double value = -1.0, mean_weight = -1.0;
    float pairs[4] = {-1.f, -1.f, -1.f, -1.f};
    if (ecc_metric_evaluate_variance(0x0, 1.f, &value, &mean_weight, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_variance(0x0, 1.f, 0x0, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_variance_transforms(0x0, 1, 1, I.data(), 1.f, &value, &mean_weight, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || mean_weight != -1.0 || pairs[0] != -1.f || pairs[3] != -1.f) return 1;
    // the host helper through the adapter: the positive entries are 1, 2, 4, 8
    std::vector<float> v(6);
    v[1] = 4.f, v[2] = -1.f, v[3] = 1.f, v[4] = 2.f, v[5] = 8.f;
    if (EpipolarConsistency::MetricRadonIntermediate::varianceFloor(v, 0.5) != 1.5f) return 1;
    bool refused = false;
    try {
        EpipolarConsistency::MetricRadonIntermediate::varianceFloor(std::vector<float>(3, 0.f));
    } catch (const std::exception&) {
        refused = true;
    }
    if (!refused) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&variance;
    return 0;
}
