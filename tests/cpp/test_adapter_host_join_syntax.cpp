// Syntax / type check (g++ -fsyntax-only -Wall -Werror -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never
// linked, never run) of the adapter's setHostJoin in its Eigen branch: it chains like the other switches of
// MetricRadonIntermediate and leaves the optimiser's two calls (Gui/SingleImageMotion.h:84-90) as they are.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double use(std::vector<Geometry::ProjectionMatrix>& Ps, std::vector<EpipolarConsistency::RadonIntermediate*>& dtrs)
{
    EpipolarConsistency::MetricRadonIntermediate ecc(Ps, dtrs);
    EpipolarConsistency::MetricRadonIntermediate& same = ecc.setRecordReuse(true, true).setHostJoin(false).setHostJoin();
    same.setProjectionMatrices(Ps);
    return same.evaluate();
}

}  // namespace

int main() { return sizeof(&use) ? 0 : 1; }
