// The adapter's RadonIntermediate::lineWeights: compiled and linked with -Wall -Werror by tests/test_line_weights_abi.py.
// Without arguments the driver only checks what needs no device and exits with 2; the function below is there to be compiled.
#include "EpipolarConsistencyHip.hxx"

#include <cstdio>
#include <memory>

namespace {

// a weight intermediate per call form: the defaults, every parameter, a context of the caller's
double weights(const std::vector<float>& flagged, int n_u, int n_v, ecc_ctx* ctx)
{
    typedef EpipolarConsistency::RadonIntermediate RI;
    std::unique_ptr<RI> a(RI::lineWeights(flagged.data(), n_u, n_v, 96, 96));
    std::unique_ptr<RI> b(RI::lineWeights(flagged.data(), n_u, n_v, 96, 96, 2.5f, 2, 3));
    std::unique_ptr<RI> c(RI::lineWeights(flagged.data(), n_u, n_v, 96, 96, 1.0f, 1, 0, ctx));
    return (a->getFilter() == RI::None) + b->getRadonBinNumber(0) + c->getRadonBinNumber(1);
}

}  // namespace

int main(int argc, char** argv)
{
    // the C entry points through the adapter's include: a null context is an argument error, nothing is launched or written
    ecc_line_weights_config cfg;
    ecc_line_weights_defaults(&cfg);
    if (cfg.dilate_px != 0 || cfg.guard_bins != 1 || cfg.zero_at_px != 1.0f) return 1;
    float image[4] = {0.f, 1.f, 0.f, 0.f}, slab[4] = {-1.f, -1.f, -1.f, -1.f};
    ecc_dtr* const untouched = reinterpret_cast<ecc_dtr*>(slab);
    ecc_dtr* out = untouched;
    if (ecc_radon_line_weights(0x0, image, 0, 1, 2, 2, 4, 4, &cfg, &out) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_radon_line_weights_into(0x0, image, 1, 2, 2, 4, 4, 0x0, slab) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (ecc_dtr_line_weights(0x0, 0x0, &cfg, &out) != ECC_ERR_INVALID_ARGUMENT) return 1;
    if (out != untouched || slab[0] != -1.f || slab[3] != -1.f) return 1;
    if (argc < 2) {
        std::printf("usage: %s run   (needs a device)\n", argv[0]);
        return 2;
    }
    (void)&weights;
    return 0;
}
