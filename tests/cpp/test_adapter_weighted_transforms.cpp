// The adapter's evaluateWeightedTransforms, non-Eigen branch: compiled and linked with -Wall -Werror by
// tests/test_weighted_transforms_abi.py.  Without arguments the driver only checks what needs no device and exits with 2; the
// function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// a Registration3D3D-shaped caller whose second scan is truncated: a population of transforms per cost call, weighted
double weighted_registration(EpipolarConsistency::MetricRadonIntermediate& ecc, int n_source, int n_target)
{
    std::vector<Geometry::RP3Homography> Ts(3);
    Ts[1](0, 3) = 6.0;   // a translation
    Ts[2](1, 3) = -3.0;
    std::vector<double> values, coverages;
    std::vector<float> terms(2 * Ts.size() * (size_t)n_source * (size_t)n_target);
    ecc.evaluateWeightedTransforms(n_source, Ts, values);
    ecc.evaluateWeightedTransforms(n_source, Ts, values, &coverages);
    ecc.evaluateWeightedTransforms(n_source, Ts, values, &coverages, terms.data());
    ecc.evaluateWeightedTransforms(n_source, Ts, values, 0x0, terms.data());
    return values[0] + values[2] + coverages[1] + terms[0] + terms[1] + (double)ecc.lastBatchedTransforms();
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry point through the adapter's include: a null metric is an argument error, nothing is launched or written
    Geometry::RP3Homography I;
    double value = -1.0, coverage = -1.0;
    float terms[2] = {-1.f, -1.f};
    if (ecc_metric_evaluate_weighted_transforms(0x0, 1, 1, I.data(), &value, &coverage, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_weighted_transforms(0x0, 1, 0, 0x0, 0x0, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || coverage != -1.0 || terms[0] != -1.f || terms[1] != -1.f) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&weighted_registration;
    return 0;
}
