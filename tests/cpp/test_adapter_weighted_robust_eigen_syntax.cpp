// Syntax / type check of the adapter's evaluateWeightedRobust, evaluateWeightedRobustPairs (both index forms) and weightedRobustScale
// in its Eigen branch (g++ -fsyntax-only -Wall -Werror -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never
// linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double weighted_robust(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<int> idx(4, 0);
    idx[1] = idx[3] = 1;
    std::vector<Eigen::Vector4i> tuples(1);
    for (int k = 0; k < 4; ++k) tuples[0][k] = idx[k];
    double coverage = 0.0, mass = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateWeightedRobust(ECC_LOSS_HUBER, 1.f) + ecc.evaluateWeightedRobust(ECC_LOSS_TRUNCATED, 1.f, &coverage) +
               ecc.evaluateWeightedRobust(ECC_LOSS_GEMAN_MCCLURE, 1.f, &coverage, &mass, &terms);
    v += ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 1.f) + ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 1.f, &coverage, &mass, &terms);
    v += ecc.evaluateWeightedRobustPairs(tuples, ECC_LOSS_HUBER, 1.f) +
         ecc.evaluateWeightedRobustPairs(tuples, ECC_LOSS_HUBER, 1.f, &coverage, &mass, &terms);
    return v + coverage + mass + terms[0] + EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(terms) +
           EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(terms, 1.4826);
}

}  // namespace

int main() { return (int)sizeof(&weighted_robust); }
