// The adapter's evaluateWeighted, non-Eigen branch: compiled and linked with -Wall -Werror by tests/test_weighted_abi.py.
// Without arguments the driver only checks what needs no device and exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// the weighted metric in its three forms: the value alone, with the coverage, with the pair terms
double weighted(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    double coverage = 0.0;
    std::vector<float> pairs;
    double v = ecc.evaluateWeighted();
    v += ecc.evaluateWeighted(&coverage);
    v += ecc.evaluateWeighted(&coverage, &pairs);
    v += ecc.evaluateWeighted(0x0, &pairs);
    return v + coverage + (pairs.empty() ? 0.0 : pairs[0] + pairs[1]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry point through the adapter's include: a null metric is an argument error, nothing is launched or written
    double value = -1.0, coverage = -1.0;
    float pairs[4] = {-1.f, -1.f, -1.f, -1.f};
    if (ecc_metric_evaluate_weighted(0x0, &value, &coverage, pairs) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_weighted(0x0, 0x0, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || coverage != -1.0 || pairs[0] != -1.f || pairs[3] != -1.f) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&weighted;
    return 0;
}
