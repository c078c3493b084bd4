// Syntax / type check of the adapter's evaluateVariance* in its Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run): Geometry::RP3Homography is
// Eigen::Matrix<double, 4, 4> there, as in the reference's Registration3D3D.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double variance(EpipolarConsistency::MetricRadonIntermediate& ecc, int n_source, float floor)
{
    std::vector<Eigen::Matrix<double, 4, 4> > Ts(2);
    for (int k = 0; k < 2; ++k)
        for (int d = 0; d < 4; ++d) Ts[k](d, d) = 1.0;
    Ts[1](0, 3) = 6.0;
    const std::vector<Geometry::RP3Homography>& same_type = Ts;
    std::vector<double> values, mean_weights;
    std::vector<float> terms(2 * 2 * 4), pairs;
    double mean_weight = 0.0;
    double v = ecc.evaluateVariance(floor, &mean_weight, &pairs);
    v += ecc.evaluateVariancePairs(std::vector<int>(4, 0), floor);
    std::vector<std::vector<int> > moved_views(1, std::vector<int>(1, 0));
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(1, std::vector<Geometry::ProjectionMatrix>(1));
    ecc.evaluateVariancePoseDeltas(moved_views, moved_Ps, floor, values, &mean_weights);
    ecc.evaluateVarianceTransforms(n_source, same_type, floor, values);
    ecc.evaluateVarianceTransforms(n_source, same_type, floor, values, &mean_weights, terms.data());
    return v + values[0] + mean_weights[1] + terms[0];
}

}  // namespace

int main() { return (int)sizeof(&variance); }
