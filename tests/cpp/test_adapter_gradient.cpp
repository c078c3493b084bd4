// The adapter's finite-difference gradient entry point (evaluateGradient / lastGradientPath), non-Eigen branch: compiled and
// linked with -Wall -Werror by tests/test_gradient_abi.py.  Without arguments the driver only checks what needs no device and
// exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// an NLopt LD_*-shaped objective: the value is returned, grad is filled
double objective(EpipolarConsistency::MetricRadonIntermediate& ecc, int view, const Geometry::ProjectionMatrix& P, double* grad_out)
{
    std::vector<double> h(6, 0.5), grad, probes;
    std::vector<Geometry::ProjectionMatrix> plus(6, P), minus(6, P);
    for (int p = 0; p < 6; ++p) {
        Geometry::RP3Homography T;
        T(p % 3, 3) = h[p];
        ecc_host_compose_transform(P.data(), T.data(), plus[p].data());
        T(p % 3, 3) = -h[p];
        ecc_host_compose_transform(P.data(), T.data(), minus[p].data());
    }
    const double value = ecc.evaluateGradient(view, plus, minus, h, grad);
    const double again = ecc.evaluateGradient(view, plus, minus, h, grad, &probes);
    for (int p = 0; p < 6; ++p) grad_out[p] = grad[p];
    return value + again + probes[0] + (double)ecc.lastGradientPath();
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null metric is an argument error, nothing is launched
    int path = -1;
    double g = 0.0;
    if (ecc_metric_evaluate_gradient(0x0, 0, 1, &g, &g, &g, 0x0, &g, 0x0) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_metric_last_gradient_path(0x0, &path) != ECC_ERR_INVALID_ARGUMENT || path != -1) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    EpipolarConsistency::MetricRadonIntermediate ecc;
    if (ecc.lastGradientPath() != 0) return 1;  // no handle yet
    (void)&objective;
    return 0;
}
