// The adapter's evaluateRobust, evaluateRobustPairs and robustScale, non-Eigen branch: compiled and linked with -Wall -Werror by
// tests/test_robust_abi.py.  Without arguments the driver only checks what needs no device and exits with 2; the functions below
// are there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

double robust_all(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    double mass = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateRobust(ECC_LOSS_HUBER, 2.5f);
    v += ecc.evaluateRobust(ECC_LOSS_TRUNCATED, 2.5f, &mass);
    v += ecc.evaluateRobust(ECC_LOSS_GEMAN_MCCLURE, 2.5f, &mass, &terms);
    v += ecc.evaluateRobust(ECC_LOSS_HUBER, (float)EpipolarConsistency::MetricRadonIntermediate::robustScale(terms, 1.5), 0x0, &terms);
    return v + mass + (terms.empty() ? 0.0 : terms[0] + terms[1] + terms[2]);
}

double robust_pairs(EpipolarConsistency::MetricRadonIntermediate& ecc)
{
    std::vector<int> idx;
    for (int q = 0; q < 3; ++q) {
        const int t[4] = {q, q + 1, q, q + 1};
        idx.insert(idx.end(), t, t + 4);
    }
    double mass = 0.0;
    std::vector<float> terms;
    double v = ecc.evaluateRobustPairs(idx, ECC_LOSS_HUBER, 2.5f);
    v += ecc.evaluateRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, &mass);
    v += ecc.evaluateRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, &mass, &terms);
    v += ecc.evaluateRobustPairs(idx, ECC_LOSS_HUBER, 2.5f, 0x0, &terms);
    return v + mass + (terms.empty() ? 0.0 : terms[0] + terms[1] + terms[2]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched or written
    const int32_t idx[4] = {0, 1, 0, 1};
    double value = -1.0, mass = -1.0;
    float terms[3] = {-1.f, -1.f, -1.f};
    if (ecc_metric_evaluate_robust(0x0, ECC_LOSS_HUBER, 1.f, &value, &mass, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_robust_pairs(0x0, idx, 1, ECC_LOSS_HUBER, 1.f, &value, &mass, terms) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (value != -1.0 || mass != -1.0 || terms[0] != -1.f || terms[1] != -1.f || terms[2] != -1.f) return 1;
    // the static scale needs no metric: rows {c, u, r} with sqrt(r) = 2, 3 -> 2.5; three floats per pair or an exception
    std::vector<float> rows(6, 1.f);
    rows[2] = 4.f;
    rows[5] = 9.f;
    if (EpipolarConsistency::MetricRadonIntermediate::robustScale(rows) != 2.5) return 1;
    if (EpipolarConsistency::MetricRadonIntermediate::robustScale(std::vector<float>()) != 0.0) return 1;
    rows.push_back(1.f);
    bool thrown = false;
    try {
        EpipolarConsistency::MetricRadonIntermediate::robustScale(rows);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    if (!thrown) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&robust_all;
    (void)&robust_pairs;
    return 0;
}
