// Syntax / type check of the adapter's evaluateVarianceRobust* in its Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run): Geometry::RP3Homography is
// Eigen::Matrix<double, 4, 4> there, as in the reference's Registration3D3D, and index lists may be Eigen::Vector4i.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double variance_robust(EpipolarConsistency::MetricRadonIntermediate& ecc, int n_source, float delta, float floor)
{
    std::vector<Eigen::Matrix<double, 4, 4> > Ts(2);
    for (int k = 0; k < 2; ++k)
        for (int d = 0; d < 4; ++d) Ts[k](d, d) = 1.0;
    Ts[1](0, 3) = 6.0;
    const std::vector<Geometry::RP3Homography>& same_type = Ts;
    std::vector<double> values, mean_weights, inlier_masses;
    std::vector<float> terms(4 * 2 * 4), pairs;
    double mean_weight = 0.0, inlier_mass = 0.0;
    double v = ecc.evaluateVarianceRobust(ECC_LOSS_TRUNCATED, delta, floor, &mean_weight, &inlier_mass, &pairs);
    v += ecc.evaluateVarianceRobustPairs(std::vector<int>(4, 0), ECC_LOSS_HUBER, delta, floor);
    v += ecc.evaluateVarianceRobustPairs(std::vector<Eigen::Vector4i>(2), ECC_LOSS_HUBER, delta, floor, &mean_weight, &inlier_mass, &pairs);
    std::vector<std::vector<int> > moved_views(1, std::vector<int>(1, 0));
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(1, std::vector<Geometry::ProjectionMatrix>(1));
    ecc.evaluateVarianceRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_GEMAN_MCCLURE, delta, floor, values, &mean_weights, &inlier_masses);
    ecc.evaluateVarianceRobustTransforms(n_source, same_type, ECC_LOSS_TRUNCATED, delta, floor, values);
    ecc.evaluateVarianceRobustTransforms(n_source, same_type, ECC_LOSS_TRUNCATED, delta, floor, values, &mean_weights, &inlier_masses, terms.data());
    return v + values[0] + mean_weights[1] + inlier_masses[1] + terms[0] + EpipolarConsistency::MetricRadonIntermediate::varianceRobustScale(pairs);
}

}  // namespace

int main() { return (int)sizeof(&variance_robust); }
