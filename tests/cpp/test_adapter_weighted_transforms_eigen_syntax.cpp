// Syntax / type check of the adapter's evaluateWeightedTransforms in its Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run): Geometry::RP3Homography is
// Eigen::Matrix<double, 4, 4> there, as in the reference's Registration3D3D.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double weighted_registration(EpipolarConsistency::MetricRadonIntermediate& ecc, int n_source)
{
    std::vector<Eigen::Matrix<double, 4, 4> > Ts(2);
    for (int k = 0; k < 2; ++k)
        for (int d = 0; d < 4; ++d) Ts[k](d, d) = 1.0;
    Ts[1](0, 3) = 6.0;
    const std::vector<Geometry::RP3Homography>& same_type = Ts;
    std::vector<double> values, coverages;
    std::vector<float> terms(2 * 2 * 4);
    ecc.evaluateWeightedTransforms(n_source, same_type, values);
    ecc.evaluateWeightedTransforms(n_source, same_type, values, &coverages);
    ecc.evaluateWeightedTransforms(n_source, same_type, values, &coverages, terms.data());
    return values[0] + coverages[1] + terms[0];
}

}  // namespace

int main() { return (int)sizeof(&weighted_registration); }
