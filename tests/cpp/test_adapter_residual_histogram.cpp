// The adapter's evaluateResidualHistogram[Pairs], evaluateVarianceResidualHistogram[Pairs] and histogramQuantile, non-Eigen branch:
// compiled and linked with -Wall -Werror by tests/test_cpp_adapter_residual_histogram.py.  Without arguments the driver only checks
// what needs no device and exits with 2.  With
//   <images.f32> n n_u n_v n_alpha n_t <matrices.f64> <pixel-variances.f32> floor width
// (raw float32 stacks of the images and of their pixel variances and n x 12 float64 matrices written by the pytest driver) it
// computes the data and the variance intermediates, builds the adapter's n and 2 n metrics and C metrics over the same
// intermediates, and prints how many results of the adapter's methods differ from what the C calls return for the same arguments.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace EpipolarConsistency;

namespace {

bool same_counts(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b)
{
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), sizeof(uint64_t) * a.size()));
}

bool read_floats(const char* path, std::vector<float>& out)
{
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(out.data(), sizeof(float), out.size(), f) == out.size();
    if (f) fclose(f);
    return ok;
}

int run(char** argv)
{
    const int n = atoi(argv[2]), n_u = atoi(argv[3]), n_v = atoi(argv[4]), n_alpha = atoi(argv[5]), n_t = atoi(argv[6]);
    const float floor = (float)atof(argv[9]), width = (float)atof(argv[10]);
    std::vector<float> imgs((size_t)n * n_u * n_v), vars(imgs.size());
    std::vector<double> Pflat(12 * (size_t)n);
    if (!read_floats(argv[1], imgs) || !read_floats(argv[8], vars)) return 3;
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(Pflat.data(), sizeof(double), Pflat.size(), f) != Pflat.size()) return 3;
    fclose(f);
    std::vector<RadonIntermediate*> data, both;
    std::vector<ProjectionMatrix> Ps(n);
    for (int k = 0; k < n; ++k) {
        data.push_back(new RadonIntermediate(imgs.data() + (size_t)k * n_u * n_v, n_u, n_v, n_alpha, n_t, RadonIntermediate::Derivative,
                                             RadonIntermediate::Identity));
        for (int e = 0; e < 12; ++e) Ps[k].data()[e] = Pflat[12 * k + e];
    }
    both = data;
    for (int k = 0; k < n; ++k)
        both.push_back(new RadonIntermediate(vars.data() + (size_t)k * n_u * n_v, n_u, n_v, n_alpha, n_t, RadonIntermediate::None,
                                             RadonIntermediate::Identity));
    std::vector<ecc_dtr*> handles;
    for (size_t k = 0; k < both.size(); ++k) handles.push_back(both[k]->handle());
    MetricRadonIntermediate* const raw = new MetricRadonIntermediate(Ps, data);   // (deleted before the dtrs they borrow)
    MetricRadonIntermediate* const var = new MetricRadonIntermediate(Ps, both);
    ecc_metric *c_raw = 0x0, *c_var = 0x0;
    detail::check(ecc_metric_create(detail::default_context(), n, handles.data(), &c_raw));
    detail::check(ecc_metric_set_projections(c_raw, Pflat.data(), n));
    detail::check(ecc_metric_create(detail::default_context(), 2 * n, handles.data(), &c_var));
    detail::check(ecc_metric_set_projections(c_var, Pflat.data(), n));

    std::vector<int> idx;
    std::vector<int32_t> idx32;
    for (int q = 0; q < 3; ++q) {
        const int t[4] = {q, q + 2, q, q + 2};
        idx.insert(idx.end(), t, t + 4);
        idx32.insert(idx32.end(), t, t + 4);
    }
    int differ = 0;
    uint64_t samples = 0;
    const int sizes[2] = {64, 256};
    for (int s = 0; s < 2; ++s) {
        const int B = sizes[s];
        std::vector<uint64_t> got, want((size_t)n * B, 7);
        raw->evaluateResidualHistogram(width, B, got);
        detail::check(ecc_metric_evaluate_residual_histogram(c_raw, width, B, want.data()));
        differ += !same_counts(got, want);
        uint64_t total = 0;
        for (size_t k = 0; k < got.size(); ++k) total += got[k];
        differ += total == 0 || (samples && total != samples);
        samples = total;
        // the median of all samples from the summed rows, by the adapter and by the C helper
        std::vector<uint64_t> row(B, 0);
        for (int v = 0; v < n; ++v)
            for (int k = 0; k < B; ++k) row[k] += got[(size_t)v * B + k];
        const double median = MetricRadonIntermediate::histogramQuantile(row, width, 0.5);
        differ += !(median > 0.0) || median != ecc_host_histogram_quantile(row.data(), B, width, 0.5);
        if (s == 0) printf("median |d| %.9g of %llu samples\n", median, (unsigned long long)(total / 2));
        raw->evaluateResidualHistogramPairs(idx, width, B, got);
        std::fill(want.begin(), want.end(), (uint64_t)7);
        detail::check(ecc_metric_evaluate_residual_histogram_pairs(c_raw, idx32.data(), 3, width, B, want.data()));
        differ += !same_counts(got, want);
        var->evaluateVarianceResidualHistogram(floor, 0.25f, B, got);
        std::fill(want.begin(), want.end(), (uint64_t)7);
        detail::check(ecc_metric_evaluate_variance_residual_histogram(c_var, floor, 0.25f, B, want.data()));
        differ += !same_counts(got, want);
        var->evaluateVarianceResidualHistogramPairs(idx, floor, 0.25f, B, got);
        std::fill(want.begin(), want.end(), (uint64_t)7);
        detail::check(ecc_metric_evaluate_variance_residual_histogram_pairs(c_var, idx32.data(), 3, floor, 0.25f, B, want.data()));
        differ += !same_counts(got, want);
        // an empty list: all zeros, written completely
        raw->evaluateResidualHistogramPairs(std::vector<int>(), width, B, got);
        for (size_t k = 0; k < got.size(); ++k) differ += got[k] != 0;
        differ += got.size() != (size_t)n * B;
    }
    printf("histograms: %d results differ\n", differ);
    // a refused argument reaches the caller as an exception with the library's text
    int thrown = 0;
    std::vector<uint64_t> got;
    try {
        raw->evaluateResidualHistogram(width, 96, got);
    } catch (const std::exception&) {
        ++thrown;
    }
    try {
        raw->evaluateVarianceResidualHistogram(floor, 0.25f, 64, got);   // n_dtrs != 2 n_views
    } catch (const std::exception&) {
        ++thrown;
    }
    printf("refused: %d of 2\n", thrown);
    detail::check(ecc_metric_destroy(c_raw));
    detail::check(ecc_metric_destroy(c_var));
    delete raw;
    delete var;
    for (size_t k = 0; k < both.size(); ++k) delete both[k];
    printf("residual histogram adapter ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    const int32_t idx[4] = {0, 1, 0, 1};
    uint64_t counts[64];
    for (int k = 0; k < 64; ++k) counts[k] = 7;
    if (ecc_metric_evaluate_residual_histogram(0x0, 1.f, 64, counts) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_residual_histogram_pairs(0x0, idx, 1, 1.f, 64, counts) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_variance_residual_histogram(0x0, 1.f, 1.f, 64, counts) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_variance_residual_histogram_pairs(0x0, idx, 1, 1.f, 1.f, 64, counts) != ECC_ERR_INVALID_ARGUMENT) return 1;
    for (int k = 0; k < 64; ++k)
        if (counts[k] != 7) return 1;
    // the host helper through the adapter
    std::vector<uint64_t> row;
    row.push_back(10), row.push_back(30), row.push_back(40), row.push_back(20);
    if (MetricRadonIntermediate::histogramQuantile(row, 0.5, 0.5) != 1.125) return 1;
    if (MetricRadonIntermediate::histogramQuantile(row, 0.5, 0.9) <= 1e300) return 1;   // the overflow bin: +infinity
    if (MetricRadonIntermediate::histogramQuantile(std::vector<uint64_t>(), 0.5, 0.5) != 0.0) return 1;
    if (argc < 11) {
        std::printf("usage: %s <images.f32> n n_u n_v n_alpha n_t <matrices.f64> <pixel-variances.f32> floor width   (needs a device)\n", argv[0]);
        return 2;
    }
    try {
        return run(argv);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 4;
    }
}
