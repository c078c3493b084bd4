// Syntax / type check of the adapter's evaluateWeighted in its Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double weighted(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    double coverage = 0.0;
    std::vector<float> pairs;
    const double v = ecc.evaluateWeighted() + ecc.evaluateWeighted(&coverage) + ecc.evaluateWeighted(&coverage, &pairs);
    return v + coverage + pairs[0];
}

}  // namespace

int main() { return (int)sizeof(&weighted); }
