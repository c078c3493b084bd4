// The adapter's evaluateVarianceRobustMap, evaluateVarianceRobustMapPairs and varianceRobustMapVariances, non-Eigen branch: compiled
// and linked with -Wall -Werror by tests/test_cpp_adapter_variance_robust_map.py.  Without arguments the driver only checks what
// needs no device and exits with 2.  With
//   <images.f32> n n_u n_v n_alpha n_t <matrices.f64> <pixel-variances.f32> floor
// (raw float32 stacks of the images and of their pixel variances and n x 12 float64 matrices written by the pytest driver) it
// computes the data and the variance intermediates, builds the adapter's 2 n metric and a C metric over the same intermediates, and
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

bool read_floats(const char* path, std::vector<float>& out)
{
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(out.data(), sizeof(float), out.size(), f) == out.size();
    if (f) fclose(f);
    return ok;
}

int run(int argc, char** argv)
{
    const int n = atoi(argv[2]), n_u = atoi(argv[3]), n_v = atoi(argv[4]), n_alpha = atoi(argv[5]), n_t = atoi(argv[6]);
    const float floor = (float)atof(argv[9]);
    std::vector<float> imgs((size_t)n * n_u * n_v), vars(imgs.size());
    std::vector<double> Pflat(12 * (size_t)n);
    if (!read_floats(argv[1], imgs) || !read_floats(argv[8], vars)) return 3;
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(Pflat.data(), sizeof(double), Pflat.size(), f) != Pflat.size()) return 3;
    fclose(f);
    (void)argc;
    std::vector<RadonIntermediate*> both;
    std::vector<ProjectionMatrix> Ps(n);
    for (int k = 0; k < n; ++k) {
        both.push_back(new RadonIntermediate(imgs.data() + (size_t)k * n_u * n_v, n_u, n_v, n_alpha, n_t, RadonIntermediate::Derivative,
                                             RadonIntermediate::Identity));
        for (int e = 0; e < 12; ++e) Ps[k].data()[e] = Pflat[12 * k + e];
    }
    for (int k = 0; k < n; ++k)   // the variance of a line integral of independent pixels: the plain transform of the pixel variances
        both.push_back(new RadonIntermediate(vars.data() + (size_t)k * n_u * n_v, n_u, n_v, n_alpha, n_t, RadonIntermediate::None,
                                             RadonIntermediate::Identity));
    std::vector<ecc_dtr*> handles;
    for (size_t k = 0; k < both.size(); ++k) handles.push_back(both[k]->handle());
    MetricRadonIntermediate* const adapter = new MetricRadonIntermediate(Ps, both);  // (deleted before the dtrs it borrows)
    MetricRadonIntermediate& ecc = *adapter;
    ecc_metric* c = 0x0;
    detail::check(ecc_metric_create(detail::default_context(), 2 * n, handles.data(), &c));
    detail::check(ecc_metric_set_projections(c, Pflat.data(), n));

    // the scale, in sigmas, from the rows without the loss
    std::vector<float> terms;
    ecc.evaluateVarianceRobust(ECC_LOSS_TRUNCATED, HUGE_VALF, floor, 0x0, 0x0, &terms);
    const float delta = (float)MetricRadonIntermediate::varianceRobustScale(terms, 2.0);
    printf("floor %.9g delta %.9g\n", floor, delta);

    const size_t bins = (size_t)n_alpha * n_t, n_pairs = (size_t)n * (n - 1) / 2;
    int differ = 0;
    std::vector<int> some;
    some.push_back(n - 1);
    some.push_back(1);
    const int32_t some32[2] = {n - 1, 1};
    for (int loss = ECC_LOSS_HUBER; loss <= ECC_LOSS_GEMAN_MCCLURE; ++loss) {
        // every view
        std::vector<float> hits, rej, rows, want_h(n * bins, -1.f), want_r(n * bins, -1.f), want_rows(4 * n_pairs, -1.f);
        double weight = -1.0, mass = -1.0, want_v = -1.0, want_w = -1.0, want_m = -1.0;
        const double v = ecc.evaluateVarianceRobustMap(loss, delta, floor, std::vector<int>(), &hits, &rej, &weight, &mass, &rows);
        detail::check(ecc_metric_evaluate_variance_robust_map(c, loss, delta, floor, 0x0, 0, want_h.data(), want_r.data(), &want_v, &want_w, &want_m,
                                                              want_rows.data()));
        differ += (v != want_v) + (weight != want_w) + (mass != want_m) + !same_floats(hits, want_h) + !same_floats(rej, want_r) +
                  !same_floats(rows, want_rows);
        // two views, unordered; only the REJ planes wanted
        std::vector<float> rej2, want_r2(2 * bins, -1.f);
        const double v2 = ecc.evaluateVarianceRobustMap(loss, delta, floor, some, 0x0, &rej2);
        detail::check(ecc_metric_evaluate_variance_robust_map(c, loss, delta, floor, some32, 2, 0x0, want_r2.data(), &want_v, 0x0, 0x0, 0x0));
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
        const double lv = ecc.evaluateVarianceRobustMapPairs(idx, loss, delta, floor, some, &lh, &lr, &weight, &mass, &lrows);
        detail::check(ecc_metric_evaluate_variance_robust_map_pairs(c, idx32.data(), 3, loss, delta, floor, some32, 2, want_lh.data(), want_lr.data(),
                                                                    &want_v, &want_w, &want_m, want_lrows.data()));
        differ += (lv != want_v) + (weight != want_w) + (mass != want_m) + !same_floats(lh, want_lh) + !same_floats(lr, want_lr) +
                  !same_floats(lrows, want_lrows);
    }
    printf("maps: %d results differ\n", differ);

    // the held map (the list call's, two views) as the next pass's variance fields: the adapter's against the C call's, read back
    differ = 0;
    std::vector<RadonIntermediate*> vs = ecc.varianceRobustMapVariances(floor, 1.0f, 1.5f, 100.0f);
    ecc_dtr* want_vs[2] = {0x0, 0x0};
    detail::check(ecc_metric_variance_robust_map_variances(c, floor, 1.0f, 1.5f, 100.0f, want_vs));
    differ += vs.size() != 2;
    for (size_t k = 0; k < vs.size() && k < 2; ++k) {
        std::vector<float> got(bins, -1.f), want(bins, -2.f);
        detail::check(ecc_dtr_readback(vs[k]->handle(), got.data()));
        detail::check(ecc_dtr_readback(want_vs[k], want.data()));
        differ += !same_floats(got, want) + (vs[k]->getFilter() != RadonIntermediate::None);
    }
    // the two weights calls refuse a map made in sigma units
    ecc_dtr* refused[2] = {0x0, 0x0};
    differ += ecc_metric_robust_map_weights(c, 1.0f, 1.5f, refused) != ECC_ERR_INVALID_ARGUMENT;
    differ += ecc_metric_weighted_robust_map_weights(c, 1.0f, 1.5f, refused) != ECC_ERR_INVALID_ARGUMENT;
    differ += refused[0] != 0x0 || refused[1] != 0x0;
    printf("variances: %d results differ, %d handles\n", differ, (int)vs.size());
    for (size_t k = 0; k < vs.size(); ++k) delete vs[k];
    for (int k = 0; k < 2; ++k) detail::check(ecc_dtr_destroy(want_vs[k]));
    detail::check(ecc_metric_destroy(c));
    delete adapter;
    for (size_t k = 0; k < both.size(); ++k) delete both[k];
    printf("variance robust map adapter ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    const int32_t idx[4] = {0, 1, 0, 1}, views[1] = {0};
    double value = -1.0, weight = -1.0, mass = -1.0;
    float terms[4] = {-1.f, -1.f, -1.f, -1.f}, plane[4] = {-1.f, -1.f, -1.f, -1.f};
    ecc_dtr* out[1] = {0x0};
    if (ecc_metric_evaluate_variance_robust_map(0x0, ECC_LOSS_HUBER, 1.f, 1.f, views, 1, plane, plane, &value, &weight, &mass, terms) !=
        ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_evaluate_variance_robust_map_pairs(0x0, idx, 1, ECC_LOSS_HUBER, 1.f, 1.f, 0x0, 0, plane, plane, &value, &weight, &mass, terms) !=
        ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_variance_robust_map_variances(0x0, 1.f, 1.f, 1.f, 1e4f, out) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || weight != -1.0 || mass != -1.0 || terms[0] != -1.f || terms[3] != -1.f || plane[0] != -1.f || plane[3] != -1.f || out[0])
        return 1;
    if (argc < 10) {
        std::printf("usage: %s <images.f32> n n_u n_v n_alpha n_t <matrices.f64> <pixel-variances.f32> floor   (needs a device)\n", argv[0]);
        return 2;
    }
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 4;
    }
}
