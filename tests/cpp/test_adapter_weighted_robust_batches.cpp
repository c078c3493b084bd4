// The adapter's evaluateWeightedRobustPoseDeltas and evaluateWeightedRobustTransforms, non-Eigen branch: compiled and linked with
// -Wall -Werror by tests/test_cpp_adapter_weighted_robust_batches.py.  Without arguments the driver only checks what needs no device
// and exits with 2.  With
//   <images.f32> n n_u n_v n_alpha n_t <matrices.f64>
// (a raw float32 image stack and n x 12 float64 matrices written by the pytest driver) it computes the intermediates and, per view,
// line weights from a flagged block (RadonIntermediate::lineWeights), builds the adapter's metric and a C metric over the same 2 n
// intermediates, and prints how many results of the two adapter methods differ from what the C calls return for the same arguments.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace EpipolarConsistency;

namespace {

bool same_bits(const std::vector<double>& a, const std::vector<double>& b)
{
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), sizeof(double) * a.size()));
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
    std::vector<RadonIntermediate*> dtrs(2 * (size_t)n);
    std::vector<ecc_dtr*> handles(2 * (size_t)n);
    std::vector<ProjectionMatrix> Ps(n);
    for (int k = 0; k < n; ++k) {
        dtrs[k] = new RadonIntermediate(imgs.data() + (size_t)k * n_u * n_v, n_u, n_v, n_alpha, n_t, RadonIntermediate::Derivative,
                                        RadonIntermediate::Identity);
        // a collimator blade: a block at the image's left edge whose width changes from view to view
        std::vector<float> flagged((size_t)n_u * n_v, 0.f);
        for (int v = 0; v < n_v; ++v)
            for (int u = 0; u < n_u / 8 + 2 * k; ++u) flagged[(size_t)v * n_u + u] = 1.f;
        dtrs[n + k] = RadonIntermediate::lineWeights(flagged.data(), n_u, n_v, n_alpha, n_t);
        for (int e = 0; e < 12; ++e) Ps[k].data()[e] = Pflat[12 * k + e];
    }
    for (size_t k = 0; k < dtrs.size(); ++k) handles[k] = dtrs[k]->handle();
    MetricRadonIntermediate* const adapter = new MetricRadonIntermediate(Ps, dtrs);  // (deleted before the dtrs it borrows)
    MetricRadonIntermediate& ecc = *adapter;
    ecc_metric* c = 0x0;
    detail::check(ecc_metric_create(detail::default_context(), 2 * n, handles.data(), &c));
    detail::check(ecc_metric_set_projections(c, Pflat.data(), n));

    // delta from the base's rows, so that about half the pairs have residuals beyond it
    std::vector<float> terms;
    double base_coverage = 0.0;
    ecc.evaluateWeightedRobust(ECC_LOSS_HUBER, HUGE_VALF, &base_coverage, 0x0, &terms);
    const float delta = (float)MetricRadonIntermediate::weightedRobustScale(terms, 0.5);
    printf("delta %.9g coverage %.9g\n", delta, base_coverage);

    // poses: one view, two views, the base itself, the last view -- each moved matrix is the view's own times a small translation
    const int lists[4][2] = {{1, -1}, {2, n - 2}, {-1, -1}, {n - 1, -1}};
    std::vector<std::vector<int> > moved_views(4);
    std::vector<std::vector<ProjectionMatrix> > moved_Ps(4);
    std::vector<int32_t> off(1, 0), views;
    std::vector<double> flat;
    for (int k = 0; k < 4; ++k) {
        for (int q = 0; q < 2 && lists[k][q] >= 0; ++q) {
            const int v = lists[k][q];
            ProjectionMatrix P = Ps[v];  // column-major: the last column becomes P (tx, ty, 0, 1)^T
            for (int r = 0; r < 3; ++r) P.data()[9 + r] += 0.4 * (k + 1) * P.data()[r] - 0.3 * P.data()[3 + r];
            moved_views[k].push_back(v);
            moved_Ps[k].push_back(P);
            views.push_back(v);
            flat.insert(flat.end(), P.data(), P.data() + 12);
        }
        off.push_back((int32_t)views.size());
    }
    int differ = 0;
    for (int loss = ECC_LOSS_HUBER; loss <= ECC_LOSS_GEMAN_MCCLURE; ++loss) {
        std::vector<double> values, coverages, masses, only, want_v(4, -1.0), want_c(4, -1.0), want_m(4, -1.0);
        ecc.evaluateWeightedRobustPoseDeltas(moved_views, moved_Ps, loss, delta, values, &coverages, &masses);
        ecc.evaluateWeightedRobustPoseDeltas(moved_views, moved_Ps, loss, delta, only);
        detail::check(ecc_metric_evaluate_weighted_robust_pose_deltas(c, 4, off.data(), views.data(), flat.data(), loss, delta, want_v.data(),
                                                                      want_c.data(), want_m.data()));
        differ += !same_bits(values, want_v) + !same_bits(coverages, want_c) + !same_bits(masses, want_m) + !same_bits(only, want_v);
        for (int k = 0; k < 4; ++k)
            differ += !(masses[k] > 0.0 && masses[k] <= 1.0 && coverages[k] > 0.0 && coverages[k] < 1.0 && values[k] > 0.0);
    }
    printf("pose deltas: %d results differ\n", differ);

    const int n_source = n / 2, n_target = n - n_source;
    std::vector<Geometry::RP3Homography> Ts(3);
    Ts[1](0, 3) = 6.0;  // translations
    Ts[2](1, 3) = -3.0;
    std::vector<double> Tflat(16 * Ts.size());
    for (size_t k = 0; k < Ts.size(); ++k)
        for (int q = 0; q < 16; ++q) Tflat[16 * k + q] = Ts[k].data()[q];
    const size_t rows = Ts.size() * (size_t)n_source * (size_t)n_target;
    differ = 0;
    for (int loss = ECC_LOSS_HUBER; loss <= ECC_LOSS_GEMAN_MCCLURE; ++loss) {
        std::vector<double> values, coverages, masses, only, want_v(Ts.size(), -1.0), want_c(Ts.size(), -1.0), want_m(Ts.size(), -1.0);
        std::vector<float> got_t(4 * rows, -1.f), want_t(4 * rows, -2.f);
        ecc.evaluateWeightedRobustTransforms(n_source, Ts, loss, delta, values, &coverages, &masses, got_t.data());
        ecc.evaluateWeightedRobustTransforms(n_source, Ts, loss, delta, only);
        detail::check(ecc_metric_evaluate_weighted_robust_transforms(c, n_source, (int)Ts.size(), Tflat.data(), loss, delta, want_v.data(),
                                                                     want_c.data(), want_m.data(), want_t.data()));
        differ += !same_bits(values, want_v) + !same_bits(coverages, want_c) + !same_bits(masses, want_m) + !same_bits(only, want_v);
        differ += std::memcmp(got_t.data(), want_t.data(), sizeof(float) * got_t.size()) != 0;
    }
    printf("transforms: %d results differ, %lld batched\n", differ, ecc.lastBatchedTransforms());
    detail::check(ecc_metric_destroy(c));
    delete adapter;
    for (size_t k = 0; k < dtrs.size(); ++k) delete dtrs[k];
    printf("weighted robust batches adapter ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    Geometry::RP3Homography I;
    const int32_t off[2] = {0, 1}, views[1] = {0};
    const double P[12] = {0};
    double value = -1.0, coverage = -1.0, mass = -1.0;
    float terms[4] = {-1.f, -1.f, -1.f, -1.f};
    if (ecc_metric_evaluate_weighted_robust_pose_deltas(0x0, 1, off, views, P, ECC_LOSS_HUBER, 1.f, &value, &coverage, &mass) != ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_evaluate_weighted_robust_transforms(0x0, 1, 1, I.data(), ECC_LOSS_HUBER, 1.f, &value, &coverage, &mass, terms) !=
        ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (ecc_metric_evaluate_weighted_robust_transforms(0x0, 1, 0, 0x0, ECC_LOSS_HUBER, 1.f, 0x0, 0x0, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || coverage != -1.0 || mass != -1.0 || terms[0] != -1.f || terms[1] != -1.f || terms[2] != -1.f || terms[3] != -1.f) return 1;
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
