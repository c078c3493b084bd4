// The adapter's evaluateGram, non-Eigen branch: compiled and linked with -Wall -Werror by tests/test_gram_abi.py.  Without
// arguments the driver only checks what needs no device and exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// the closed-form value of a coefficient vector under the Gram matrix of a K-channel metric
double form(EpipolarConsistency::MetricRadonIntermediate& ecc, int K, const std::vector<double>& a)
{
    std::vector<double> G;
    std::vector<float> pairs;
    ecc.evaluateGram(K, G);
    ecc.evaluateGram(K, G, &pairs);
    double v = 0.0;
    for (int c = 0; c < K; ++c)
        for (int d = 0; d < K; ++d) v += a[c] * G[(size_t)c * K + d] * a[d];
    return v + (pairs.empty() ? 0.0 : (double)pairs[0]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry point through the adapter's include: a null metric and a null result are argument errors, nothing is launched
    double G[4] = {-1.0, -1.0, -1.0, -1.0};
    if (ecc_metric_evaluate_gram(0x0, 2, 0x0, G) != ECC_ERR_INVALID_ARGUMENT || G[0] != -1.0) return 1;
    if (ecc_metric_evaluate_gram(0x0, 2, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&form;
    return 0;
}
