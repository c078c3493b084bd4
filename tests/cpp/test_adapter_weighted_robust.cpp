// The adapter's evaluateWeightedRobust, evaluateWeightedRobustPairs and weightedRobustScale, non-Eigen branch: compiled and linked
// with -Wall -Werror by tests/test_cpp_adapter_weighted_robust.py.  Without arguments the driver only checks what needs no device and
// exits with 2; the functions below are there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

double weighted_robust_all(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    double coverage = 0.0, mass = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateWeightedRobust(ECC_LOSS_HUBER, 2.5f);
    v += ecc.evaluateWeightedRobust(ECC_LOSS_TRUNCATED, 2.5f, &coverage);
    v += ecc.evaluateWeightedRobust(ECC_LOSS_GEMAN_MCCLURE, 2.5f, &coverage, &mass);
    v += ecc.evaluateWeightedRobust(ECC_LOSS_GEMAN_MCCLURE, 2.5f, &coverage, &mass, &terms);
    v += ecc.evaluateWeightedRobust(ECC_LOSS_HUBER, (float)EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(terms, 1.5), 0x0,
                                    0x0, &terms);
    return v + coverage + mass + (terms.empty() ? 0.0 : terms[0] + terms[1] + terms[2] + terms[3]);
}

double weighted_robust_pairs(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<int> idx;
    for (int q = 0; q < 3; ++q) {
        const int t[4] = {q, q + 1, q, q + 1};
        idx.insert(idx.end(), t, t + 4);
    }
    double coverage = 0.0, mass = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 2.5f);
    v += ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, &coverage);
    v += ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, &coverage, &mass);
    v += ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, &coverage, &mass, &terms);
    v += ecc.evaluateWeightedRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, 0x0, 0x0, &terms);
    return v + coverage + mass + (terms.empty() ? 0.0 : terms[0] + terms[1] + terms[2] + terms[3]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    const int32_t idx[4] = {0, 1, 0, 1};
    double value = -1.0, coverage = -1.0, mass = -1.0;
    float terms[4] = {-1.f, -1.f, -1.f, -1.f};
    if (ecc_metric_evaluate_weighted_robust(0x0, ECC_LOSS_HUBER, 1.f, &value, &coverage, &mass, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_weighted_robust_pairs(0x0, idx, 1, ECC_LOSS_HUBER, 1.f, &value, &coverage, &mass, terms) != ECC_ERR_INVALID_ARGUMENT)
        return 1;
    if (value != -1.0 || coverage != -1.0 || mass != -1.0 || terms[0] != -1.f || terms[1] != -1.f || terms[2] != -1.f || terms[3] != -1.f) return 1;
    // the static scale needs no metric: rows {c, u, k, r} with sqrt(r / u) = 2, 3 -> 2.5; four floats per pair or an exception
    std::vector<float> rows(8, 1.f);
    rows[3] = 4.f;
    rows[5] = 0.25f;
    rows[7] = 2.25f;
    if (EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(rows) != 2.5) return 1;
    if (EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(std::vector<float>()) != 0.0) return 1;
    // with u == 1 it is robustScale of the rows {c, k, r}
    std::vector<float> four(8, 1.f), three(6, 1.f);
    four[3] = three[2] = 7.f;
    four[7] = three[5] = 3.f;
    if (EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(four, 1.4826) != EpipolarConsistency::MetricRadonIntermediate::robustScale(three, 1.4826))
        return 1;
    rows.push_back(1.f);
    bool thrown = false;
    try {
        EpipolarConsistency::MetricRadonIntermediate::weightedRobustScale(rows);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&weighted_robust_all;
    (void)&weighted_robust_pairs;
    return 0;
}
