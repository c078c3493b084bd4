// ecc_studentised_weight.h -- the weight of one sample under inverse-variance weights and a robust loss in sigma units, stated once
// for variance_robust_kernel.hip (which sums om and f) and variance_robust_map_kernel.hip (which also deposits 1 - w): both take it
// through FieldLossForm under StudentisedRule, ecc_loss_forms.h.  Device code only; every line one float32 operation:
//   s   = V_a + V_b
//   sc  = s < floor ? floor : s
//   om  = 1.0f / sc                       the correctly rounded IEEE division
//   a   = fabsf(d)
//   huber, truncated    thr = delta * sqrtf(sc);  t = fminf(1.0f, thr / a);   w = t * (2.0f - t)  |  t * t
//   geman-mcclure       q = a * inv_delta;        w = 1.0f / fmaf(q * om, q, 1.0f)
//   f   = om * w
#ifndef ECC_STUDENTISED_WEIGHT_H
#define ECC_STUDENTISED_WEIGHT_H

#include "ecc_layout.h"

namespace {

// the launch-uniform part of the weight, in scalar registers
struct StudentisedLoss {
    int loss;
    float delta, inv_delta, floor;
};

// the two factors of a sample's weight f = om * w, and w, the loss weight of the studentised residual, alone
struct StudentisedWeight {
    float om, f, w;
};

// om = 1 / max(V_a + V_b, floor) and f = om * w(|d| / sqrt(max(V_a + V_b, floor))) (`loss` is wave-uniform, the branch a scalar one)
__device__ __forceinline__ StudentisedWeight studentised_weight(const StudentisedLoss& L, float va, float vb, float d)
{
    const float s = va + vb;
    const float sc = s < L.floor ? L.floor : s;
    const float om = 1.0f / sc;
    const float a = fabsf(d);
    float w;
    if (L.loss == ECC_ROBUST_GEMAN_MCCLURE) {
        const float q = a * L.inv_delta;
        w = 1.0f / fmaf(q * om, q, 1.0f);
    } else {
        const float thr = L.delta * sqrtf(sc);
        const float t = fminf(1.0f, thr / a);
        w = L.loss == ECC_ROBUST_HUBER ? t * (2.0f - t) : t * t;
    }
    return {om, om * w, w};
}

}  // namespace

#endif
