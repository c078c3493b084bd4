// The adapter's registration entry point and the two virtuals of the reference's Metric interface that its base lacked
// (ref: LibEpipolarConsistency/EpipolarConsistency.h:76,85-87), non-Eigen branch: compiled and linked with -Wall -Werror by
// tests/test_cpp_adapter_transforms.py.  Without arguments the driver only checks what needs no device and exits with 2;
// the functions below it are there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>

namespace {

// code that holds the interface only, as the reference's callers do
double through_the_base(EpipolarConsistency::Metric& metric, int i, int j)
{
    std::vector<UtilsCuda::BindlessTexture2D<float>*> no_textures;
    metric.setProjectionImages(no_textures);  // a stub in the reference too
    std::vector<float> s0, s1, kappas;
    return metric.evaluateForImagePair(i, j, &s0, &s1, &kappas) + metric.evaluateForImagePair(i, j);
}

// a Registration3D3D-shaped caller: a population of transforms per cost call
double registration(EpipolarConsistency::MetricRadonIntermediate& ecc, int n_source, int n_target)
{
    std::vector<Geometry::RP3Homography> Ts(3);
    Ts[1](0, 3) = 6.0;   // a translation
    Ts[2](1, 3) = -3.0;
    std::vector<double> means;
    std::vector<float> values(Ts.size() * (size_t)n_source * (size_t)n_target);
    ecc.evaluateTransforms(n_source, Ts, means);
    ecc.evaluateTransforms(n_source, Ts, means, values.data());
    return means[0] + means[1] + means[2] + values[0] + (double)ecc.lastBatchedTransforms();
}

}  // namespace

int main(int argc, char** argv)
{
    // the identity by default, column-major
    Geometry::RP3Homography I;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            if (I(r, c) != (r == c ? 1.0 : 0.0) || I.data()[r + 4 * c] != I(r, c)) return 1;
    // ecc_host_compose_transform through the header: P times the identity is P, bit for bit
    Geometry::ProjectionMatrix P, Q;
    for (int k = 0; k < 12; ++k) P.data()[k] = 0.1 * (k + 1);
    ecc_host_compose_transform(P.data(), I.data(), Q.data());
    for (int k = 0; k < 12; ++k)
        if (P.data()[k] != Q.data()[k]) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    // both derived classes are still instantiable, and usable through the base
    EpipolarConsistency::MetricRadonIntermediate ecc;
    EpipolarConsistency::Metric& base = ecc;
    (void)base;
    (void)&through_the_base;
    (void)&registration;
    return 0;
}
