// Syntax / type check of the Eigen branch of the adapter's gradient entry point (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run): Geometry::ProjectionMatrix is
// Eigen::Matrix<double, 3, 4> there, as in the reference's SingleImageMotion.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double gradient(EpipolarConsistency::MetricRadonIntermediate& ecc, int view)
{
    std::vector<Eigen::Matrix<double, 3, 4> > plus(6), minus(6);
    const std::vector<Geometry::ProjectionMatrix>& same_type = plus;
    std::vector<double> h(6, 0.5), grad, probes;
    const double value = ecc.evaluateGradient(view, same_type, minus, h, grad);
    return value + ecc.evaluateGradient(view, plus, minus, h, grad, &probes) + grad[0] + probes[11] + ecc.lastGradientPath();
}

}  // namespace

int main() { return (int)sizeof(&gradient); }
