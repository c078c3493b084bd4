// Syntax / type check of the adapter's setFormIncremental and lastFormBasePairs (g++ -fsyntax-only -Wall -Werror; never linked,
// never run), in both branches of the adapter: with -DECC_TEST_MOCK_EIGEN and tests/cpp/mock_eigen on the include path the Eigen
// branch, with -DECC_TEST_PLAIN_BRANCH and no Eigen on the path the plain one.  The switch chains like the other switches of
// MetricRadonIntermediate, and the counter is a const member.
#include "EpipolarConsistencyHip.hxx"

#if defined(ECC_TEST_MOCK_EIGEN) && !defined(ECC_ADAPTER_HAVE_EIGEN)
#error "the adapter did not take its Eigen branch"
#endif
#if defined(ECC_TEST_PLAIN_BRANCH) && defined(ECC_ADAPTER_HAVE_EIGEN)
#error "the adapter did not take its plain branch"
#endif

namespace {

long long use(std::vector<Geometry::ProjectionMatrix>& Ps, std::vector<EpipolarConsistency::RadonIntermediate*>& dtrs)
{
    EpipolarConsistency::MetricRadonIntermediate ecc(Ps, dtrs);
    EpipolarConsistency::MetricRadonIntermediate& same = ecc.setFormIncremental().setHostJoin(true).setFormIncremental(false).setFormIncremental(true);
    same.setProjectionMatrices(Ps);
    std::vector<std::vector<int> > moved_views(1, std::vector<int>(1, 0));
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(1, std::vector<Geometry::ProjectionMatrix>(1));
    std::vector<double> values;
    same.evaluateRobustPoseDeltas(moved_views, moved_Ps, ECC_LOSS_HUBER, 2.5f, values);
    const EpipolarConsistency::MetricRadonIntermediate& read_only = same;
    return read_only.lastFormBasePairs();
}

}  // namespace

int main() { return sizeof(&use) ? 0 : 1; }
