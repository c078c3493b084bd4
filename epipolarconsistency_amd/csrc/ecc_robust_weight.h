// ecc_robust_weight.h -- the IRLS weight of a residual under a robust loss, stated once for the forms that take one (RobustForm
// and FieldLossForm under LineWeightRule, ecc_loss_forms.h: the robust and weighted-robust kernel files and their maps).  Every loss is rho(d) = w(d) d^2 with w in (0, 1], one float32 operation per line,
// nothing contracted but the fmaf, the division the IEEE one (the head of robust_kernel.hip has the table).
#ifndef ECC_ROBUST_WEIGHT_H
#define ECC_ROBUST_WEIGHT_H

#include "ecc_layout.h"

namespace {

// the launch-uniform part of the loss
struct RobustLoss {
    int loss;
    float delta, inv_delta;
};

// w(d): the IRLS weight of a residual (`loss` is wave-uniform, the branch a scalar one)
__device__ __forceinline__ float robust_weight(const RobustLoss& L, float d)
{
    const float a = fabsf(d);
    if (L.loss == ECC_ROBUST_GEMAN_MCCLURE) {
        const float s = a * L.inv_delta;
        return 1.0f / fmaf(s, s, 1.0f);
    }
    const float t = fminf(1.0f, L.delta / a);
    return L.loss == ECC_ROBUST_HUBER ? t * (2.0f - t) : t * t;
}

}  // namespace

#endif
