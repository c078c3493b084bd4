// Syntax / type check of the adapter's evaluateGram in its Eigen branch (g++ -fsyntax-only -Wall -Werror -DECC_TEST_MOCK_EIGEN
// with tests/cpp/mock_eigen on the include path; never linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double gram(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<double> G;
    std::vector<float> pairs;
    ecc.evaluateGram(3, G);
    ecc.evaluateGram(3, G, &pairs);
    return G[0] + G[8] + (double)pairs[0];
}

}  // namespace

int main() { return (int)sizeof(&gram); }
