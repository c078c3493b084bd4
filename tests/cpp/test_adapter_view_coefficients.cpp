// The adapter's evaluateViewCoefficients, non-Eigen branch: compiled and linked with -Wall -Werror by
// tests/test_view_coefficients_abi.py.  Without arguments the driver only checks what needs no device and exits with 2; the
// function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// one step of gradient descent over the per-view coefficients of a K-channel metric
double descend(EpipolarConsistency::MetricRadonIntermediate& ecc, int K, std::vector<float>& a, double step)
{
    std::vector<double> grad;
    std::vector<float> pairs;
    const double before = ecc.evaluateViewCoefficients(K, a);
    ecc.evaluateViewCoefficients(K, a, &grad);
    ecc.evaluateViewCoefficients(K, a, &grad, &pairs);
    for (size_t k = 0; k < a.size(); ++k) a[k] -= (float)(step * grad[k]);
    return before - ecc.evaluateViewCoefficients(K, a) + (pairs.empty() ? 0.0 : (double)pairs[0]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry point through the adapter's include: null arguments are argument errors, nothing is launched or written
    const float a[4] = {1.f, 1.f, 1.f, 1.f};
    double value = -1.0, grad[4] = {-1.0, -1.0, -1.0, -1.0};
    if (ecc_metric_evaluate_view_coefficients(0x0, 2, a, &value, grad, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_view_coefficients(0x0, 2, a, 0x0, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || grad[0] != -1.0) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&descend;
    return 0;
}
