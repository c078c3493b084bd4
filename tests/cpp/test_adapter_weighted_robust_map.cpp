// The adapter's evaluateWeightedRobustMap, evaluateWeightedRobustMapPairs and weightedRobustMapWeights, non-Eigen branch: compiled
// and linked with -Wall -Werror by tests/test_cpp_adapter_weighted_robust_map.py.  Without arguments the driver only checks what
// needs no device and exits with 2.  With
//   <images.f32> n n_u n_v n_alpha n_t <matrices.f64>
// (a raw float32 image stack and n x 12 float64 matrices written by the pytest driver) it computes the intermediates, takes a first
// set of line weights from the n-metric's map, builds the adapter's 2 n metric and a C metric over the same intermediates, and
// prints how many results of the adapter's methods differ from what the C calls return for the same arguments.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace EpipolarConsistency;

namespace {

bool same_floats(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), sizeof(float) * a.size()));
}

int run(int argc, char** argv)
{
    const int n = atoi(argv[2]), n_u = atoi(argv[3]), n_v = atoi(argv[4]), n_alpha = atoi(argv[5]), n_t = atoi(argv[6]);
    std::vector<float> imgs((size_t)n * n_u * n_v);
    std::vector<double> Pflat(12 * (size_t)n);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(imgs.data(), sizeof(float), imgs.size(), f) != imgs.size()) return 3;
    fclose(f);
    f = fopen(argv[7], "rb");
    if (!f || fread(Pflat.data(), sizeof(double), Pflat.size(), f) != Pflat.size()) return 3;
    fclose(f);
    (void)argc;
    std::vector<RadonIntermediate*> dtrs;
    std::vector<ProjectionMatrix> Ps(n);
    for (int k = 0; k < n; ++k) {
        dtrs.push_back(new RadonIntermediate(imgs.data() + (size_t)k * n_u * n_v, n_u, n_v, n_alpha, n_t, RadonIntermediate::Derivative,
                                             RadonIntermediate::Identity));
        for (int e = 0; e < 12; ++e) Ps[k].data()[e] = Pflat[12 * k + e];
    }
    // pass 1 on the n-metric: the scale and a first set of weights
    MetricRadonIntermediate* const plain = new MetricRadonIntermediate(Ps, dtrs);
    std::vector<float> terms;
    plain->evaluateRobust(ECC_LOSS_HUBER, HUGE_VALF, 0x0, &terms);
    const float delta = (float)MetricRadonIntermediate::robustScale(terms, 0.5);
    printf("delta %.9g\n", delta);
    plain->evaluateRobustMap(ECC_LOSS_TRUNCATED, delta, std::vector<int>(), 0x0, 0x0);
    std::vector<RadonIntermediate*> first = plain->robustMapWeights(1.0f, 1.0f);
    delete plain;
    if ((int)first.size() != n) return 5;

    std::vector<RadonIntermediate*> both(dtrs);
    both.insert(both.end(), first.begin(), first.end());
    std::vector<ecc_dtr*> handles;
    for (size_t k = 0; k < both.size(); ++k) handles.push_back(both[k]->handle());
    MetricRadonIntermediate* const adapter = new MetricRadonIntermediate(Ps, both);  // (deleted before the dtrs it borrows)
    MetricRadonIntermediate& ecc = *adapter;
    ecc_metric* c = 0x0;
    detail::check(ecc_metric_create(detail::default_context(), 2 * n, handles.data(), &c));
    detail::check(ecc_metric_set_projections(c, Pflat.data(), n));

    const size_t bins = (size_t)n_alpha * n_t, n_pairs = (size_t)n * (n - 1) / 2;
    int differ = 0;
    std::vector<int> some;
    some.push_back(n - 1);
    some.push_back(1);
    const int32_t some32[2] = {n - 1, 1};
    for (int loss = ECC_LOSS_HUBER; loss <= ECC_LOSS_GEMAN_MCCLURE; ++loss) {
        // every view
        std::vector<float> hits, rej, rows, want_h(n * bins, -1.f), want_r(n * bins, -1.f), want_rows(4 * n_pairs, -1.f);
        double cover = -1.0, mass = -1.0, want_v = -1.0, want_c = -1.0, want_m = -1.0;
        const double v = ecc.evaluateWeightedRobustMap(loss, delta, std::vector<int>(), &hits, &rej, &cover, &mass, &rows);
        detail::check(ecc_metric_evaluate_weighted_robust_map(c, loss, delta, 0x0, 0, want_h.data(), want_r.data(), &want_v, &want_c, &want_m,
                                                              want_rows.data()));
        differ += (v != want_v) + (cover != want_c) + (mass != want_m) + !same_floats(hits, want_h) + !same_floats(rej, want_r) +
                  !same_floats(rows, want_rows);
        // two views, unordered; only the REJ planes wanted
        std::vector<float> rej2, want_r2(2 * bins, -1.f);
        const double v2 = ecc.evaluateWeightedRobustMap(loss, delta, some, 0x0, &rej2);
        detail::check(ecc_metric_evaluate_weighted_robust_map(c, loss, delta, some32, 2, 0x0, want_r2.data(), &want_v, 0x0, 0x0, 0x0));
        differ += (v2 != want_v) + !same_floats(rej2, want_r2) + (std::memcmp(rej2.data(), rej.data() + (size_t)(n - 1) * bins, sizeof(float) * bins) != 0);
        // the list form over three pairs
        std::vector<int> idx;
        std::vector<int32_t> idx32;
        for (int q = 0; q < 3; ++q) {
            const int t[4] = {q, q + 2, q, q + 2};
            idx.insert(idx.end(), t, t + 4);
            idx32.insert(idx32.end(), t, t + 4);
        }
        std::vector<float> lh, lr, lrows, want_lh(2 * bins, -1.f), want_lr(2 * bins, -1.f), want_lrows(12, -1.f);
        const double lv = ecc.evaluateWeightedRobustMapPairs(idx, loss, delta, some, &lh, &lr, &cover, &mass, &lrows);
        detail::check(ecc_metric_evaluate_weighted_robust_map_pairs(c, idx32.data(), 3, loss, delta, some32, 2, want_lh.data(), want_lr.data(),
                                                                    &want_v, &want_c, &want_m, want_lrows.data()));
        differ += (lv != want_v) + (cover != want_c) + (mass != want_m) + !same_floats(lh, want_lh) + !same_floats(lr, want_lr) +
                  !same_floats(lrows, want_lrows);
    }
    printf("maps: %d results differ\n", differ);

    // the held map (the list call's, two views) as the next pass's weights: the adapter's against the C call's, read back
    differ = 0;
    std::vector<RadonIntermediate*> ws = ecc.weightedRobustMapWeights(1.0f, 1.5f);
    ecc_dtr* want_ws[2] = {0x0, 0x0};
    detail::check(ecc_metric_weighted_robust_map_weights(c, 1.0f, 1.5f, want_ws));
    differ += ws.size() != 2;
    for (size_t k = 0; k < ws.size() && k < 2; ++k) {
        std::vector<float> got(bins, -1.f), want(bins, -2.f);
        detail::check(ecc_dtr_readback(ws[k]->handle(), got.data()));
        detail::check(ecc_dtr_readback(want_ws[k], want.data()));
        differ += !same_floats(got, want) + (ws[k]->getFilter() != RadonIntermediate::None);
    }
    // the n-metric's weights call refuses a map made under line weights
    ecc_dtr* refused[2] = {0x0, 0x0};
    differ += ecc_metric_robust_map_weights(c, 1.0f, 1.5f, refused) != ECC_ERR_INVALID_ARGUMENT;
    printf("weights: %d results differ, %d handles\n", differ, (int)ws.size());
    for (size_t k = 0; k < ws.size(); ++k) delete ws[k];
    for (int k = 0; k < 2; ++k) detail::check(ecc_dtr_destroy(want_ws[k]));
    detail::check(ecc_metric_destroy(c));
    delete adapter;
    for (size_t k = 0; k < both.size(); ++k) delete both[k];
    printf("weighted robust map adapter ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    const int32_t idx[4] = {0, 1, 0, 1}, views[1] = {0};
    double value = -1.0, cover = -1.0, mass = -1.0;
    float terms[4] = {-1.f, -1.f, -1.f, -1.f}, plane[4] = {-1.f, -1.f, -1.f, -1.f};
    ecc_dtr* out[1] = {0x0};
    if (ecc_metric_evaluate_weighted_robust_map(0x0, ECC_LOSS_HUBER, 1.f, views, 1, plane, plane, &value, &cover, &mass, terms) !=
        ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_evaluate_weighted_robust_map_pairs(0x0, idx, 1, ECC_LOSS_HUBER, 1.f, 0x0, 0, plane, plane, &value, &cover, &mass, terms) !=
        ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_weighted_robust_map_weights(0x0, 1.f, 1.f, out) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || cover != -1.0 || mass != -1.0 || terms[0] != -1.f || terms[3] != -1.f || plane[0] != -1.f || plane[3] != -1.f || out[0])
        return 1;
    if (argc < 8) {
        std::printf("usage: %s <images.f32> n n_u n_v n_alpha n_t <matrices.f64>   (needs a device)\n", argv[0]);
        return 2;
    }
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 4;
    }
}
