// Syntax / type check of MetricDirect's index-list overload under the adapter's Eigen branch (g++ -fsyntax-only -Wall -Werror
// -DECC_TEST_MOCK_EIGEN with tests/cpp/mock_eigen on the include path; never linked, never run): the objective of
// Gui/SingleImageMotion.h written against MetricDirect -- the list (input_index, i, input_index, i) of every other view i, with
// the candidate matrix as a further row of the table -- and a batch of candidates through evaluatePoseDeltas.
#include "EpipolarConsistencyHip.hxx"

#ifndef ECC_ADAPTER_HAVE_EIGEN
#error "the adapter did not take its Eigen branch"
#endif

namespace {

double one_view_objective(EpipolarConsistency::MetricDirect& ecc, std::vector<Geometry::ProjectionMatrix> Ps, int input_index,
                          const Geometry::ProjectionMatrix& candidate)
{
    const int n = ecc.getNumberOfProjetions();
    Ps.push_back(candidate);  // row n of the table
    ecc.setProjectionMatrices(Ps);
    std::vector<Eigen::Vector4i> indices;
    for (int i = 0; i < n; ++i) {
        if (i == input_index) continue;
        Eigen::Vector4i t;
        t[0] = n; t[1] = i; t[2] = input_index; t[3] = i;
        indices.push_back(t);
    }
    std::vector<float> tmp_results(indices.size());
    const double with_out = ecc.evaluate(indices, tmp_results.data());
    const double without = ecc.evaluate(indices);
    std::vector<std::vector<int> > moved_views(2, std::vector<int>(1, input_index));
    std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(2, std::vector<Geometry::ProjectionMatrix>(1, candidate));
    std::vector<double> terms;
    std::vector<int32_t> tuples;
    const std::vector<double> sums = ecc.evaluatePoseDeltas(moved_views, moved_Ps, &terms, &tuples);
    return with_out + without + sums[0] + ecc.evaluate() + tmp_results[0];
}

}  // namespace

int main() { return sizeof(&one_view_objective) ? 0 : 1; }
