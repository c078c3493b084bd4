// Syntax / type check of the adapter's evaluateWeightedRobustPoseDeltas and evaluateWeightedRobustTransforms in its Eigen branch (g++
// -fsyntax-only -Wall -Werror -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run):
// Geometry::RP3Homography is Eigen::Matrix<double, 4, 4> there, Geometry::ProjectionMatrix Eigen::Matrix<double, 3, 4>.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double weighted_robust_poses(EpipolarConsistency::MetricRadonIntermediate& ecc, const Geometry::ProjectionMatrix& P)
{
    std::vector<std::vector<int> > moved_views(2);
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(2);
    moved_views[0].push_back(1);
    moved_Ps[0].push_back(P);
    std::vector<double> values, coverages, masses;
    ecc.evaluateWeightedRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_HUBER, 2.5f, values);
    ecc.evaluateWeightedRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_TRUNCATED, 2.5f, values, &coverages);
    ecc.evaluateWeightedRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_GEMAN_MCCLURE, 2.5f, values, &coverages, &masses);
    ecc.evaluateWeightedRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_GEMAN_MCCLURE, 2.5f, values, 0x0, &masses);
    return values[0] + coverages[0] + masses[1];
}

double weighted_robust_registration(EpipolarConsistency::MetricRadonIntermediate& ecc, int n_source)
{
    std::vector<Eigen::Matrix<double, 4, 4> > Ts(2);
    for (int k = 0; k < 2; ++k)
        for (int d = 0; d < 4; ++d) Ts[k](d, d) = 1.0;
    Ts[1](0, 3) = 6.0;
    const std::vector<Geometry::RP3Homography>& same_type = Ts;
    std::vector<double> values, coverages, masses;
    std::vector<float> terms(2 * 3 * 4 * 4);
    ecc.evaluateWeightedRobustTransforms(n_source, same_type, ECC_LOSS_TRUNCATED, 2.5f, values);
    ecc.evaluateWeightedRobustTransforms(n_source, same_type, ECC_LOSS_TRUNCATED, 2.5f, values, &coverages);
    ecc.evaluateWeightedRobustTransforms(n_source, same_type, ECC_LOSS_TRUNCATED, 2.5f, values, &coverages, &masses);
    ecc.evaluateWeightedRobustTransforms(n_source, same_type, ECC_LOSS_TRUNCATED, 2.5f, values, &coverages, &masses, terms.data());
    return values[0] + coverages[0] + masses[1] + terms[0];
}

}  // namespace

int main() { return (int)(sizeof(&weighted_robust_poses) + sizeof(&weighted_robust_registration)); }
