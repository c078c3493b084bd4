// Syntax / type check of the adapter's evaluateViewHessian in its Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double matrix(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<double> H, blocks;
    ecc.evaluateViewHessian(3, H);
    ecc.evaluateViewHessian(3, H, &blocks);
    ecc.evaluateViewPairBlocks(3, blocks);
    return H[0] + blocks[0];
}

}  // namespace

int main() { return (int)sizeof(&matrix); }
