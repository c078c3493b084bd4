// MetricDirect's index lists and pose batches through the header-only adapter (EpipolarConsistencyHip.hxx): compiled with
// g++ -std=c++11 -Wall -Werror and linked against libecc_hip.so by tests/test_direct_lists_abi.py.
//   test_direct_lists                        usage code 2, no device touched
//   test_direct_lists <file> <n> <n_u> <n_v>   <file>: n x 12 float64 matrices (column-major), then n x n_v x n_u float32 pixels;
//                                            prints the results as hexadecimal floats, which the test compares with the
//                                            Python calls' bits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "EpipolarConsistencyHip.hxx"

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const int n = std::atoi(argv[2]), n_u = std::atoi(argv[3]), n_v = std::atoi(argv[4]);
    if (n < 5) return 2;
    std::vector<double> flat(12 * (size_t)n);
    std::vector<float> images((size_t)n * n_u * n_v);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    if (std::fread(flat.data(), sizeof(double), flat.size(), f) != flat.size() ||
        std::fread(images.data(), sizeof(float), images.size(), f) != images.size())
        return 2;
    std::fclose(f);
    std::vector<Geometry::ProjectionMatrix> Ps((size_t)n);
    for (int v = 0; v < n; ++v) std::memcpy(Ps[(size_t)v].data(), &flat[12 * (size_t)v], sizeof(double) * 12);
    try {
        std::vector<Geometry::ProjectionMatrix> table(Ps);
        Geometry::ProjectionMatrix candidate;
        for (int k = 0; k < 12; ++k) candidate.data()[k] = 0.5 * (Ps[3].data()[k] + Ps[4].data()[k]);
        table.push_back(candidate);  // row n: a candidate for view 3
        EpipolarConsistency::MetricDirect ecc(table, images.data(), n, n_u, n_v);
        // the list of the moved view 3 with the candidate row (ref: Gui/SingleImageMotion.h), ascending image indices
        std::vector<int32_t> idx4;
        for (int i = 0; i < n; ++i) {
            if (i == 3) continue;
            const int32_t t[4] = {i < 3 ? i : n, i < 3 ? n : i, i < 3 ? i : 3, i < 3 ? 3 : i};
            idx4.insert(idx4.end(), t, t + 4);
        }
        std::vector<float> out((size_t)n - 1, -1.f);
        std::vector<double> values;
        const double sum = ecc.evaluate_indices(idx4.data(), n - 1, out.data(), &values);
        if (values.size() != out.size()) return 1;
        for (size_t q = 0; q < out.size(); ++q)
            if (out[q] != (float)values[q] || !(out[q] > 0)) return 1;
        if (ecc.evaluate_indices(idx4.data(), n - 1) != sum) return 1;
        std::printf("list_sum %a\nfirst_value %a\n", sum, values[0]);

        std::vector<std::vector<int> > moved_views(2);
        std::vector<std::vector<Geometry::ProjectionMatrix> > moved_Ps(2);
        moved_views[0].push_back(3);
        moved_Ps[0].push_back(candidate);
        moved_views[1].push_back(1);
        moved_views[1].push_back(3);
        moved_Ps[1].push_back(Ps[3]);
        moved_Ps[1].push_back(Ps[1]);
        std::vector<double> terms;
        std::vector<int32_t> tuples;
        const std::vector<double> sums = ecc.evaluatePoseDeltas(moved_views, moved_Ps, &terms, &tuples);
        if (sums.size() != 2 || terms.size() != (size_t)(n - 1) + (size_t)(2 * (n - 1) - 1) || tuples.size() != 4 * terms.size()) return 1;
        if (sums[0] != sum) return 1;  // pose 0 is the list above: the same pairs in the same order
        if (ecc.evaluatePoseDeltas(moved_views, moved_Ps) != sums) return 1;
        std::printf("pose_sums %a %a\nevaluate %a\nok\n", sums[0], sums[1], ecc.evaluate());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
