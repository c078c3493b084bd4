// ecc_residual_histogram.h -- what residual_histogram_kernel.hip and its host file ecc_residual_histogram.hip share: the parameters
// of the two histogram launches, the bin rule, the studentised residual and a wave's private counters.
//
// The table of a call is n_views rows of n_bins unsigned 64-bit cells, zero before the launch.  Row v receives every +-kappa sample
// of every pair that has v as one of its two data indices: a sample is counted in both rows of its pair.  The bin of a sample, every
// line one float32 operation:
//   a   = fabsf(d)                        raw form; the variance form: fabsf(d) / sqrtf(sc), sc = max(V_i + V_j, floor) as below
//   x   = a * inv_width                   inv_width = (float)(1.0 / (double)width), formed on the host
//   bin = x < (float)(n_bins - 1) ? (int)x : n_bins - 1
// The comparison is made in float BEFORE the conversion: NaN and +inf fail it and land in the last bin, the overflow bin, and no
// value of d whatever can form an index outside [0, n_bins).
#ifndef ECC_RESIDUAL_HISTOGRAM_H
#define ECC_RESIDUAL_HISTOGRAM_H

#include "ecc_layout.h"

enum { ECC_HISTOGRAM_MIN_BINS = 64, ECC_HISTOGRAM_MAX_BINS = 1024 };  // n_bins: a multiple of 64 between the two (64: a wave's lanes)

// One intermediate per view, as for pairs_kernel.
struct EccResidualHistogramParams {
    unsigned long long* counts;  // n_views rows of n_bins cells, zero before the launch
    int n_bins;
    float inv_width;             // (float)(1.0 / (double)width), finite and > 0
};

// 2 n_views channel-major intermediates and copies as for EccVarianceParams: channel 0 the data, channel 1 the variance fields.
struct EccVarianceResidualHistogramParams {
    int64_t paired_channel_bytes;  // as in EccGramParams
    int64_t quad_channel_bytes;
    unsigned long long* counts;
    int n_bins;
    float inv_width;               // width counts sigmas
    float floor;                   // as in EccVarianceParams; launch-uniform
};

// the LDS of a launch: one private table of 32-bit counters per wave of the workgroup (4 waves, main and reference kernels alike)
static inline size_t ecc_residual_histogram_lds_bytes(int n_bins) { return 4 * (size_t)n_bins * sizeof(unsigned); }

#if defined(__HIPCC__)
extern "C" hipError_t ecc_launch_pairs_residual_histogram(const EccPairParams* p, const EccResidualHistogramParams* g, hipStream_t stream);
extern "C" hipError_t ecc_launch_pairs_variance_residual_histogram(const EccPairParams* p, const EccVarianceResidualHistogramParams* g,
                                                                   hipStream_t stream);
#endif

// ---- the counters: for the kernel file, behind ecc_pair_forms.h ----------------------------------------------------------------
#if defined(ECC_PAIR_FORMS_H)
namespace {

// |z| of a sample with the residual d and the two UNSIGNED variance samples va, vb: ecc_studentised_weight.h's s and sc, then the
// correctly rounded root and division (the compiler's expansions; no intrinsic, no fast-math flag)
__device__ __forceinline__ float studentised_residual(float floor, float va, float vb, float d)
{
    const float s = va + vb;
    const float sc = s < floor ? floor : s;
    return fabsf(d) / sqrtf(sc);
}

// What orders the lanes of one wave around its counters.  A wave's LDS operations are carried out in the order they were issued, so
// the hardware needs no instruction here; the compiler does: the fences keep it from moving the zeroing stores, the atomics and the
// flush's loads across this point, and the (convergent) wave barrier from giving some lanes the code behind it while others are still
// in front of it.
__device__ __forceinline__ void wave_counters_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The private sub-histogram of one wave: n_bins 32-bit counters in the launch's dynamic LDS, wave w's behind wave w - 1's.  No other
// wave ever touches them, so no workgroup barrier is needed -- and none could be used: waves leave the kernels independently.  A pair
// has fewer than 2^31 samples (2 k_limit), so a counter cannot wrap.
struct WaveCounters {
    typedef __attribute__((address_space(3))) unsigned* Lds;
    Lds h;               // this wave's counters
    int n_bins, last;    // wave-uniform
    float inv_width, last_f;
    unsigned long long *row0, *row1;  // the pair's two rows of the table
    bool live;           // begin ran: this wave has a pair, its counters are zeroed and wait to be flushed

    __device__ __forceinline__ WaveCounters() : live(false) {}

    // once per pair, all lanes: zero the counters (lane l the bins l, l + 64, ...)
    __device__ __forceinline__ void begin(unsigned long long* counts, int bins, float inv_w, int iD0, int iD1)
    {
        extern __shared__ unsigned ecc_histogram_lds[];
        n_bins = __builtin_amdgcn_readfirstlane(bins);
        last = n_bins - 1;
        last_f = (float)last;
        inv_width = uniformf(inv_w);
        h = (Lds)ecc_histogram_lds + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * n_bins;  // (the base in a scalar register)
        row0 = counts + (long long)iD0 * n_bins;
        row1 = counts + (long long)iD1 * n_bins;
        for (int b = threadIdx.x & 63; b < n_bins; b += 64) h[b] = 0u;
        wave_counters_order();
        live = true;
    }

    // one sample with the binned quantity a >= 0 (or NaN): one LDS integer atomic, result unused
    __device__ __forceinline__ void count(float a) const
    {
        const float x = a * inv_width;
        const int bin = x < last_f ? (int)x : last;
        __hip_atomic_fetch_add(h + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }

    // behind the pair's loops, all lanes of the wave, whatever the frame returned: lane l adds the non-zero counts of the bins l,
    // l + 64, ... to the pair's two rows (plain global atomics, results unused; integer sums: the same bits in any order)
    __device__ __forceinline__ void flush() const
    {
        if (!live) return;  // wave-uniform: this wave had no pair
        wave_counters_order();
        for (int b = threadIdx.x & 63; b < n_bins; b += 64) {
            const unsigned c = h[b];
            if (c) {
                atomicAdd(row0 + b, (unsigned long long)c);
                atomicAdd(row1 + b, (unsigned long long)c);
            }
        }
    }
};

// the argument check the two launch functions share: no correlation cost, no record slots, no skip list; the table there; n_bins a
// multiple of the wave between the limits; a finite positive inv_width
template <class G>
inline bool histogram_launch_ok(const EccPairParams& p, const G& g)
{
    return !(p.use_corr || p.record_slots || p.skip_enabled || !g.counts || g.n_bins < ECC_HISTOGRAM_MIN_BINS ||
             g.n_bins > ECC_HISTOGRAM_MAX_BINS || (g.n_bins & 63) || !(g.inv_width > 0.0f) || !(g.inv_width <= FLT_MAX));
}

}  // namespace
#endif

#endif
