// Syntax / type check of the adapter's evaluateWeightedPairs and evaluateWeightedPoseDeltas in its Eigen branch (g++ -fsyntax-only
// -Wall -Werror -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run).
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double weighted_poses(EpipolarConsistency::MetricRadonIntermediate& ecc, const std::vector<Geometry::ProjectionMatrix>& Ps)
{
    std::vector<int> idx(4, 0);
    idx[1] = idx[3] = 1;
    double coverage = 0.0;
    std::vector<float> terms;
    const double v = ecc.evaluateWeightedPairs(idx) + ecc.evaluateWeightedPairs(idx, &coverage) + ecc.evaluateWeightedPairs(idx, &coverage, &terms);
    std::vector<std::vector<int> > moved(1, std::vector<int>(1, 1));
    std::vector<std::vector<Geometry::ProjectionMatrix> > mats(1, std::vector<Geometry::ProjectionMatrix>(1, Ps[1]));
    std::vector<double> values, coverages;
    ecc.evaluateWeightedPoseDeltas(moved, mats, values);
    ecc.evaluateWeightedPoseDeltas(moved, mats, values, &coverages);
    return v + coverage + terms[0] + values[0] + coverages[0];
}

}  // namespace

int main() { return (int)sizeof(&weighted_poses); }
