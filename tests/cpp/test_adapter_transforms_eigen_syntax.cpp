// Syntax / type check of the Eigen branch of the adapter's registration entry point (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run): Geometry::RP3Homography is
// Eigen::Matrix<double, 4, 4> there, as in the reference's Registration3D3D.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double registration(EpipolarConsistency::MetricRadonIntermediate& ecc, EpipolarConsistency::Metric& base, int n_source)
{
    std::vector<Eigen::Matrix<double, 4, 4> > Ts(2);
    for (int k = 0; k < 2; ++k)
        for (int d = 0; d < 4; ++d) Ts[k](d, d) = 1.0;
    Ts[1](0, 3) = 6.0;
    const std::vector<Geometry::RP3Homography>& same_type = Ts;
    std::vector<double> means;
    ecc.evaluateTransforms(n_source, same_type, means);
    std::vector<UtilsCuda::BindlessTexture2D<float>*> no_textures;
    base.setProjectionImages(no_textures);
    return means[0] + base.evaluateForImagePair(0, 1);
}

double use(EpipolarConsistency::MetricRadonIntermediate& ecc) { return registration(ecc, ecc, 1); }

}  // namespace

int main() { return (int)sizeof(&use); }
