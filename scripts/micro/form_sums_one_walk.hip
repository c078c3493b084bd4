// Micro-benchmark: the pose sum over S = 3 columns in ONE walk (sum_form_poses_kernel, csrc/form_sums_kernel.hip) against TWO launches
// of the two-column kernel (sum_weighted_poses_kernel, csrc/weighted_poses_kernel.hip) on the same buffers -- columns {0, 1}, then
// columns {2, 3} -- which is the design DESIGN.md 4.23 had planned.  Random columns; K poses that each move one view of n; the three
// sums of every pose must have the same bits either way (the program exits with 1 otherwise).  Times are HIP-event times per batch,
// the median of 9 groups of 20 launches.
//   cd epipolarconsistency_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize \
//       -o /tmp/form_sums_one_walk ../../scripts/micro/form_sums_one_walk.hip form_sums_kernel.hip weighted_poses_kernel.hip
//   /tmp/form_sums_one_walk [n K moved]...          (default: 400 600 1, 400 12 1, 130 600 1, 67 600 4)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

extern "C" hipError_t ecc_launch_sum_weighted_poses(const float* base_cols, long long base_stride, long long count, int n, int Q,
                                                    const int32_t* lists_d, int K, const float* val_cols, long long vals_stride, int slices,
                                                    double* partial_d, double* out_host_dev, hipStream_t stream);
extern "C" hipError_t ecc_launch_sum_form_poses(const float* base_cols, long long base_stride, long long count, int n, int Q,
                                                const int32_t* lists_d, int K, const float* val_cols, long long vals_stride, int S, int slices,
                                                double* partial_d, double* out_host_dev, hipStream_t stream);

#define CHECK(x)                                                                          \
    do {                                                                                  \
        const hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                           \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                           \
            std::exit(2);                                                                 \
        }                                                                                 \
    } while (0)

template <class F>
static double median_us(hipStream_t s, F&& launch)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    for (int w = 0; w < 3; ++w) launch();
    CHECK(hipStreamSynchronize(s));
    std::vector<float> us;
    for (int g = 0; g < 9; ++g) {
        CHECK(hipEventRecord(a, s));
        for (int r = 0; r < 20; ++r) launch();
        CHECK(hipEventRecord(b, s));
        CHECK(hipEventSynchronize(b));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, a, b));
        us.push_back(1e3f * ms / 20);
    }
    std::sort(us.begin(), us.end());
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return us[us.size() / 2];
}

static int run(int n, int K, int moved)
{
    if (moved < 1 || moved > 32 || n < 8 * moved || n > 4096 || K < 1 || K > 16384) {  // (the kernels hold at most 32 moved views per pose)
        std::printf("need 1 <= moved <= 32, 8 moved <= n <= 4096, 1 <= K <= 16384\n");
        return 1;
    }
    const long long count = (long long)n * (n - 1) / 2, base_stride = (count + 3) & ~3ll;
    const int Q = K * moved, slices = count >= 32768 ? 16 : 1;
    const long long vals_stride = ((long long)n * Q + 3) & ~3ll;
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> d(0.f, 1.f);
    std::vector<float> base(4 * (size_t)base_stride), vals(4 * (size_t)vals_stride);
    for (auto& v : base) v = d(rng);
    for (auto& v : vals) v = d(rng);
    std::vector<int32_t> lists((size_t)K + 1 + Q);
    for (int k = 0; k <= K; ++k) lists[k] = k * moved;
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < moved; ++a) lists[(size_t)K + 1 + k * moved + a] = (int)(((long long)(k % 7 + a * (n / moved))) % n);  // ascending
    for (int k = 0; k < K; ++k) std::sort(&lists[(size_t)K + 1 + k * moved], &lists[(size_t)K + 1 + (k + 1) * moved]);
    float *base_d, *vals_d;
    int32_t* lists_d;
    double *partial_d, *out_h, *out_dev;
    CHECK(hipMalloc(&base_d, sizeof(float) * base.size()));
    CHECK(hipMalloc(&vals_d, sizeof(float) * vals.size()));
    CHECK(hipMalloc(&lists_d, sizeof(int32_t) * lists.size()));
    CHECK(hipMalloc(&partial_d, sizeof(double) * 4 * (size_t)K * 16));
    CHECK(hipHostMalloc(&out_h, sizeof(double) * 7 * (size_t)K, hipHostMallocMapped));
    CHECK(hipHostGetDevicePointer((void**)&out_dev, out_h, 0));
    CHECK(hipMemcpy(base_d, base.data(), sizeof(float) * base.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(vals_d, vals.data(), sizeof(float) * vals.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(lists_d, lists.data(), sizeof(int32_t) * lists.size(), hipMemcpyHostToDevice));
    std::memset(out_h, 0xff, sizeof(double) * 7 * (size_t)K);
    hipStream_t s;
    CHECK(hipStreamCreate(&s));
    // words: [0, 3 K) the one walk; [3 K, 5 K) columns {0, 1}; [5 K, 7 K) columns {2, 3}
    auto one_walk = [&]() {
        CHECK(ecc_launch_sum_form_poses(base_d, base_stride, count, n, Q, lists_d, K, vals_d, vals_stride, 3, slices, partial_d, out_dev, s));
    };
    auto two_launches = [&]() {
        CHECK(ecc_launch_sum_weighted_poses(base_d, base_stride, count, n, Q, lists_d, K, vals_d, vals_stride, slices, partial_d, out_dev + 3 * (size_t)K, s));
        CHECK(ecc_launch_sum_weighted_poses(base_d + 2 * base_stride, base_stride, count, n, Q, lists_d, K, vals_d + 2 * vals_stride, vals_stride, slices,
                                            partial_d + 2 * (size_t)K * 16, out_dev + 5 * (size_t)K, s));
    };
    auto first_launch = [&]() {
        CHECK(ecc_launch_sum_weighted_poses(base_d, base_stride, count, n, Q, lists_d, K, vals_d, vals_stride, slices, partial_d, out_dev + 3 * (size_t)K, s));
    };
    const double t1 = median_us(s, one_walk), t2 = median_us(s, two_launches), t0 = median_us(s, first_launch);
    CHECK(hipStreamSynchronize(s));
    int differ = 0;
    for (int k = 0; k < K; ++k) {
        differ += std::memcmp(&out_h[3 * (size_t)k], &out_h[3 * (size_t)K + 2 * (size_t)k], 2 * sizeof(double)) != 0;
        differ += std::memcmp(&out_h[3 * (size_t)k + 2], &out_h[5 * (size_t)K + 2 * (size_t)k], sizeof(double)) != 0;
    }
    std::printf("{\"n\": %d, \"pairs\": %lld, \"K\": %d, \"moved\": %d, \"slices\": %d, \"one_walk_us\": %.2f, \"two_launches_us\": %.2f, "
                "\"two_column_launch_us\": %.2f, \"poses_that_differ\": %d}\n",
                n, count, K, moved, slices, t1, t2, t0, differ);
    CHECK(hipStreamDestroy(s));
    CHECK(hipFree(base_d));
    CHECK(hipFree(vals_d));
    CHECK(hipFree(lists_d));
    CHECK(hipFree(partial_d));
    CHECK(hipHostFree(out_h));
    return differ;
}

int main(int argc, char** argv)
{
    int bad = 0;
    if (argc >= 4) {
        for (int a = 1; a + 2 < argc; a += 3) bad += run(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]));
    } else {
        bad += run(400, 600, 1);
        bad += run(400, 12, 1);
        bad += run(130, 600, 1);
        bad += run(67, 600, 4);
    }
    return bad ? 1 : 0;
}
