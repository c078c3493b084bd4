// Syntax / type check of the adapter's evaluateRobust, evaluateRobustPairs (both index forms) and robustScale in its Eigen branch
// (g++ -fsyntax-only -Wall -Werror -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double robust(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<int> idx(4, 0);
    idx[1] = idx[3] = 1;
    std::vector<Eigen::Vector4i> tuples(1);
    for (int k = 0; k < 4; ++k) tuples[0][k] = idx[k];
    double mass = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateRobust(ECC_LOSS_HUBER, 1.f) + ecc.evaluateRobust(ECC_LOSS_TRUNCATED, 1.f, &mass) +
               ecc.evaluateRobust(ECC_LOSS_GEMAN_MCCLURE, 1.f, &mass, &terms);
    v += ecc.evaluateRobustPairs(idx, ECC_LOSS_HUBER, 1.f) + ecc.evaluateRobustPairs(idx, ECC_LOSS_HUBER, 1.f, &mass, &terms);
    v += ecc.evaluateRobustPairs(tuples, ECC_LOSS_HUBER, 1.f) + ecc.evaluateRobustPairs(tuples, ECC_LOSS_HUBER, 1.f, &mass, &terms);
    return v + mass + terms[0] + EpipolarConsistency::MetricRadonIntermediate::robustScale(terms) +
           EpipolarConsistency::MetricRadonIntermediate::robustScale(terms, 1.4826);
}

}  // namespace

int main() { return (int)sizeof(&robust); }
