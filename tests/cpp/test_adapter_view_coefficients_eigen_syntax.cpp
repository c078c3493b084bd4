// Syntax / type check of the adapter's evaluateViewCoefficients in its Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double coefficients(EpipolarConsistency::MetricRadonIntermediate& ecc, const std::vector<float>& a)
{
    std::vector<double> grad;
    std::vector<float> pairs;
    const double v = ecc.evaluateViewCoefficients(3, a);
    return v + ecc.evaluateViewCoefficients(3, a, &grad) + ecc.evaluateViewCoefficients(3, a, &grad, &pairs) + grad[0] + (double)pairs[0];
}

}  // namespace

int main() { return (int)sizeof(&coefficients); }
