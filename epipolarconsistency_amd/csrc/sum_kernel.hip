// sum_kernel.hip -- the float64 total of the pair values of an evaluation (gfx950): one workgroup, or ecc_sum::SLICES of them
// inside one launch from ecc_sum::SPLIT_MIN_COUNT values on; the column sums of the Gram form (sum_gram_kernel) and the per-view sums of
// the view-coefficient gradient (sum_view_terms_kernel).  The order
// of the additions is ecc_sum_order.h's; what is written here is how the values are fetched and how the result reaches its
// reader.
#include <hip/hip_runtime.h>

#include "ecc_sum_order.h"

namespace {

// One slice: a single workgroup, deterministic.
// values_host (optional, pinned and device-mapped): the kernel also hands the values themselves to the host -- every thread
// stores what it loads, 16 contiguous bytes per lane, drained before the barrier in front of the result's store; writes of
// one device to host memory arrive in order, so a host that sees the result sees the values (index lists: no copy command).
__global__ __launch_bounds__(ecc_sum::THREADS) void sum_pairs_kernel(const float* __restrict__ vals, long long count,
                                                                     double* __restrict__ out, float* __restrict__ values_host)
{
    constexpr int T = ecc_sum::THREADS;
    __shared__ double s[ecc_sum::WAVES];
    ecc_sum::Acc4 a;
    const long long n4 = count >> 2;
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(vals);
    if (values_host) {  // uniform; its own pass, so that the arithmetic below is the one code path it always was
        // system-scope stores (plain stores to host memory may sit in the L2 until the kernel ends; the host reads the
        // values as soon as it sees the result)
        for (long long q = threadIdx.x; q < count; q += T)
            __hip_atomic_store(reinterpret_cast<unsigned*>(values_host) + q, __float_as_uint(vals[q]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // eight loads in flight per thread: the kernel is one workgroup reading what other XCDs have just written
    // (HBM latency each time), issued one at a time it took 10 us for 79 800 values
    long long k = threadIdx.x;
    // (All of a thread's ~20 loads in flight at once would make it one round trip, but 1024 threads x 20 float4 do not fit
    // the 128 registers a thread of this workgroup may have: it spilled.  Ten per batch = two round trips.)
    for (; k + 9 * T < n4; k += 10 * T) {
        float4 v[10];
#pragma unroll
        for (int u = 0; u < 10; ++u) v[u] = v4[k + u * T];
#pragma unroll
        for (int u = 0; u < 10; ++u) ecc_sum::add(a, v[u]);
    }
    for (; k + 7 * T < n4; k += 8 * T) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = v4[k + u * T];
#pragma unroll
        for (int u = 0; u < 8; ++u) ecc_sum::add(a, v[u]);
    }
    for (; k < n4; k += T) ecc_sum::add(a, v4[k]);
    double acc = ecc_sum::combine(a);
    if (threadIdx.x == 0) ecc_sum::add_tail(acc, vals + (n4 << 2), n4, count);
    ecc_sum::stage_wave_sums(acc, s);
    if (threadIdx.x == 0) {
        const double tot = ecc_sum::waves_in_order(s);
        // `out` is usually pinned host memory that the host polls (ecc_capi.hip: wait_result): one 8-byte store at
        // system scope, written through, visible to the host before the kernel's end-of-dispatch write-back
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(out), (unsigned long long)__double_as_longlong(tot),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ecc_sum::SLICES workgroups inside ONE launch: every workgroup reduces its slice -- one memory round trip instead of the
// single workgroup's two -- and publishes its float64 partial; the workgroup that arrives last (a ticket counter) adds the
// partials in slice order and stores the result.  Deterministic whichever workgroup happens to be last.
// Hand-off between workgroups as the CDNA4 guide prescribes for it (MI355X_MICROARCH.md, "Valid forms"): the partial is an
// agent-scope (sc1, write-through) store, the storing lane drains it (s_waitcnt vmcnt(0)) before its agent-scope ticket
// add, the last arriver -- told by the value its add returned -- reads the partials with agent-scope (sc1) loads.
// That hand-off is what gfx950's code generation of these operations guarantees, not what the C++ memory model does for
// relaxed atomics: the kernel is tied to the target it was written and measured for.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "sum_pairs_split_kernel's cross-workgroup hand-off is specified for gfx950 only"
#endif
struct SumScratch {
    double partial[ecc_sum::SLICES];
    unsigned ticket;  // zero between launches (reset by the last arriver)
};
static_assert(sizeof(SumScratch) >= sizeof(double) * ecc_sum::SLICES + sizeof(unsigned), "a partial per slice and the ticket");

__global__ __launch_bounds__(ecc_sum::THREADS) void sum_pairs_split_kernel(const float* __restrict__ vals, long long count,
                                                                           double* __restrict__ out, SumScratch* __restrict__ scratch)
{
    constexpr int T = ecc_sum::THREADS, SLICES = ecc_sum::SLICES;
    __shared__ double s[ecc_sum::WAVES];
    __shared__ unsigned s_ticket;
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, SLICES, blockIdx.x, &lo, &hi);
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(vals);
    ecc_sum::Acc4 a;
    long long k = lo + threadIdx.x;
    for (; k + 3 * T < hi; k += 4 * T) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = v4[k + u * T];
#pragma unroll
        for (int u = 0; u < 4; ++u) ecc_sum::add(a, v[u]);
    }
    for (; k < hi; k += T) ecc_sum::add(a, v4[k]);
    double acc = ecc_sum::combine(a);
    if (blockIdx.x == SLICES - 1 && threadIdx.x == 0) ecc_sum::add_tail(acc, vals + (n4 << 2), n4, count);
    ecc_sum::stage_wave_sums(acc, s);
    if (threadIdx.x == 0) {
        const double part = ecc_sum::waves_in_order(s);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(&scratch->partial[blockIdx.x]),
                           (unsigned long long)__double_as_longlong(part), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_ticket = __hip_atomic_fetch_add(&scratch->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s_ticket == SLICES - 1) {  // every other workgroup's partial was drained before its add: all are visible
            double tot = 0.0;
            for (int b = 0; b < SLICES; ++b)
                tot += __longlong_as_double((long long)__hip_atomic_load(
                    reinterpret_cast<unsigned long long*>(&scratch->partial[b]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            __hip_atomic_store(&scratch->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(out), (unsigned long long)__double_as_longlong(tot),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The T column sums of ecc_metric_evaluate_gram (gram_kernel.hip) in one launch: workgroup (slice, column) adds its slice of the
// column as sum_pairs_kernel / sum_pairs_split_kernel do (ecc_sum_order.h) and stores the slice's sum; the host adds the slice
// sums to 0.0 in slice order.  The slice loop is sum_pairs_split_kernel's, statement by statement
// (kept apart: sharing changes sum_pairs_split_kernel's code, see CHANGELOG).
__global__ __launch_bounds__(ecc_sum::THREADS) void sum_gram_kernel(const float* __restrict__ values, long long col_stride, long long count,
                                                                    int n_slices, double* __restrict__ partial)
{
    constexpr int TH = ecc_sum::THREADS;
    __shared__ double s[ecc_sum::WAVES];
    const float* __restrict__ vals = values + (long long)blockIdx.y * col_stride;
    const long long n4 = count >> 2;
    long long lo, hi;
    ecc_sum::slice_bounds(n4, n_slices, blockIdx.x, &lo, &hi);
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(vals);
    ecc_sum::Acc4 a;
    long long k = lo + threadIdx.x;
    for (; k + 3 * TH < hi; k += 4 * TH) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = v4[k + u * TH];
#pragma unroll
        for (int u = 0; u < 4; ++u) ecc_sum::add(a, v[u]);
    }
    for (; k < hi; k += TH) ecc_sum::add(a, v4[k]);
    double acc = ecc_sum::combine(a);
    if ((int)blockIdx.x == n_slices - 1 && threadIdx.x == 0) ecc_sum::add_tail(acc, vals + (n4 << 2), n4, count);
    ecc_sum::stage_wave_sums(acc, s);
    if (threadIdx.x == 0) partial[(long long)blockIdx.y * ecc_sum::SLICES + blockIdx.x] = ecc_sum::waves_in_order(s);
}

// The gradient sums of ecc_metric_evaluate_view_coefficients (view_coeff_kernel.hip): workgroup (view v, channel c) adds the n - 1
// terms of the pairs that contain v -- column 1 + c (h0) of the pair (v, w) where v is the smaller index, column 1 + K + c (h1) of
// the pair (w, v) where it is the larger.  THE order, for every reader of these sums: the partners w = 0 .. n - 1 without v in
// ascending order are terms u = 0 .. n - 2; thread t adds its terms u = t, t + THREADS, ... in float64 to 0.0; the 64 threads of a
// wave are combined by ecc_sum::wave_sum's tree and the wave sums added to 0.0 in wave order (stage_wave_sums, waves_in_order).
// No atomics: the same bits on every run.
__global__ __launch_bounds__(ecc_sum::THREADS) void sum_view_terms_kernel(const float* __restrict__ values, long long col_stride, int n_views,
                                                                          int n_channels, double* __restrict__ sums)
{
    __shared__ double s[ecc_sum::WAVES];
    const int v = blockIdx.x, c = blockIdx.y;
    const float* __restrict__ h0 = values + (long long)(1 + c) * col_stride;
    const float* __restrict__ h1 = values + (long long)(1 + n_channels + c) * col_stride;
    double acc = 0.0;
    for (int u = threadIdx.x; u < n_views - 1; u += ecc_sum::THREADS) {
        const int w = u < v ? u : u + 1;
        const long long lo = w < v ? w : v, hi = w < v ? v : w;
        const long long pair = lo * n_views - lo * (lo + 1) / 2 + (hi - lo - 1);  // get_ij order (ecc_layout.h)
        acc += (double)(w < v ? h1[pair] : h0[pair]);
    }
    ecc_sum::stage_wave_sums(acc, s);
    if (threadIdx.x == 0) sums[(long long)c * n_views + v] = ecc_sum::waves_in_order(s);
}

// One double from device memory into a pinned, device-mapped host slot (system-scope store): how a value that a
// collective left on the device (the all-reduced sum of a sharded evaluation) reaches a polling host without a copy command.
__global__ void publish_scalar_kernel(const double* __restrict__ value, double* __restrict__ host_slot)
{
    const unsigned long long bits = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(value), __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_slot), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

extern "C" hipError_t ecc_launch_publish_scalar(const double* value_d, double* host_slot_dev, hipStream_t stream)
{
    hipLaunchKernelGGL(publish_scalar_kernel, dim3(1), dim3(1), 0, stream, value_d, host_slot_dev);
    return hipGetLastError();
}

extern "C" size_t ecc_sum_scratch_bytes() { return sizeof(SumScratch); }

extern "C" hipError_t ecc_launch_sum_pairs_to_host(const float* vals, long long count, double* out, float* values_host, hipStream_t stream)
{
    hipLaunchKernelGGL(sum_pairs_kernel, dim3(1), dim3(ecc_sum::THREADS), 0, stream, vals, count, out, values_host);
    return hipGetLastError();
}

// scratch: ecc_sum_scratch_bytes() of zeroed device memory owned by the caller (one per stream of launches), or null.
extern "C" hipError_t ecc_launch_sum_pairs(const float* vals, long long count, double* out, void* scratch, hipStream_t stream)
{
    if (ecc_sum::slices(count, scratch != nullptr) > 1)
        hipLaunchKernelGGL(sum_pairs_split_kernel, dim3(ecc_sum::SLICES), dim3(ecc_sum::THREADS), 0, stream, vals, count, out,
                           static_cast<SumScratch*>(scratch));
    else
        hipLaunchKernelGGL(sum_pairs_kernel, dim3(1), dim3(ecc_sum::THREADS), 0, stream, vals, count, out, (float*)nullptr);
    return hipGetLastError();
}

// partial_d: n_columns x ecc_sum::SLICES doubles; entry [t][s] = sum of slice s of column t, s < n_slices (1 or ecc_sum::SLICES).
extern "C" hipError_t ecc_launch_sum_gram(const float* values_d, long long col_stride, long long count, int n_columns, int n_slices,
                                          double* partial_d, hipStream_t stream)
{
    if (count <= 0 || n_columns < 1 || (n_slices != 1 && n_slices != ecc_sum::SLICES)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sum_gram_kernel, dim3((unsigned)n_slices, (unsigned)n_columns), dim3(ecc_sum::THREADS), 0, stream, values_d,
                       col_stride, count, n_slices, partial_d);
    return hipGetLastError();
}

// sums_d: n_channels x n_views doubles; entry [c][v] = the sum of the gradient terms of (view v, channel c) over the pairs with v.
// values_d: the 1 + 2 n_channels columns of ecc_launch_pairs_coeff for all n_views (n_views - 1) / 2 pairs.
extern "C" hipError_t ecc_launch_sum_view_terms(const float* values_d, long long col_stride, int n_views, int n_channels, double* sums_d,
                                                hipStream_t stream)
{
    if (n_views < 2 || n_channels < 1 || col_stride < (long long)n_views * (n_views - 1) / 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sum_view_terms_kernel, dim3((unsigned)n_views, (unsigned)n_channels), dim3(ecc_sum::THREADS), 0, stream, values_d,
                       col_stride, n_views, n_channels, sums_d);
    return hipGetLastError();
}
