// The adapter's evaluateViewHessian, non-Eigen branch: compiled and linked with -Wall -Werror by tests/test_view_hessian_abi.py.
// Without arguments the driver only checks what needs no device and exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// a^T H a of a K-channel metric's per-view coefficients, plus the first pair-block entry
double form(EpipolarConsistency::MetricRadonIntermediate& ecc, int K, const std::vector<double>& a)
{
    std::vector<double> H, blocks;
    ecc.evaluateViewHessian(K, H);
    ecc.evaluateViewHessian(K, H, &blocks);
    ecc.evaluateViewPairBlocks(K, blocks);
    double f = 0.0;
    for (size_t r = 0; r < a.size(); ++r)
        for (size_t c = 0; c < a.size(); ++c) f += a[r] * H[r * a.size() + c] * a[c];
    return f + (blocks.empty() ? 0.0 : blocks[0]);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry point through the adapter's include: null arguments are argument errors, nothing is launched or written
    double H[4] = {-1.0, -1.0, -1.0, -1.0}, blocks[10] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0};
    if (ecc_metric_evaluate_view_hessian(0x0, 2, H, blocks) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_evaluate_view_hessian(0x0, 2, 0x0, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (H[0] != -1.0 || blocks[0] != -1.0 || blocks[9] != -1.0) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&form;
    return 0;
}
