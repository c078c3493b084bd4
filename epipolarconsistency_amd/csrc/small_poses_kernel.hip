// small_poses_kernel.hip -- the probes of a finite-difference gradient of ONE moved view: records and sampling in ONE launch (gfx950).
//
// ecc_metric_evaluate_pose_deltas (ecc_poses.hip) spends five dependent launches on a batch -- pose_list_kernel, k01_kernel,
// pairs_kernel, sum_poses_kernel [, finish_poses_kernel] -- which is right for the hundreds of poses of a sweep and slow for the
// twelve probes of a central difference over six parameters: 79 us for ~18 us of pair-kernel work on 400 views.
// Here the first three are one kernel, built like small_eval_kernel.hip (OPT-IN, ecc_debug_set_gradient_launch: measured on one
// MI355X it takes 37-39 us for the 4 800 entries of 400 views where the three launches take about 29, and the call is no faster --
// DESIGN.md 4.11):
//   * E1 of the Q probe matrices is done by the HOST (ecc_host_geometry.h: the code e1_kernel compiles, bit-identical) and
//     handed over in the KERNEL ARGUMENTS, as entries of the EccSmallEval patch list filed under the geometry indices
//     n, n + 1, ... n + Q - 1 -- the extended-array convention of the pose batch.  The partners' geometry is what the device
//     arrays PinvTs / Cs hold (the caller has brought them up to date).  Workgroup 0 stores the entries behind the n views'
//     (k01_fit_block does): the arrays have room for ECC_SMALL_PATCH_MAX entries there (ecc_metric_set_projections).
//   * The grid is partner-major, probe-minor: entry e = u * Q + q is the pair {partner u, moved view} under probe q --
//     neighbours in the launch sample the same two Radon intermediates under slightly different geometries, their lines are
//     shared in the L1 / L2.  The entry u = moved view is a hole: a pair of view 0 with itself, value 0, which
//     nobody reads (pose_list_kernel's convention).  The index tuples are made in the kernel; there is no list.
//   * phase A: the records of the workgroup's pairs by k01_fit_block<8> -- the code of k01_kernel<8> -- into LDS;
//   * phase B: the sampling loops of pairs_kernel (pair_accumulate), four waves per workgroup: one wave per pair from 4097
//     entries on, as ecc_launch_pairs chooses, two or four waves per pair below (pairs_split_kernel's scheme: staged terms,
//     added again in one wave's order by resum_staged -- pairs_kernel's bits).  The reference arithmetic (the mode evaluations of
//     at most ECC_SAMPLING_AUTO_REFERENCE_PAIRS pairs resolve to): one pair per workgroup, the loop of pairs_reference_kernel<.., 4>;
//   * phase C: plain stores of the pair values into the slots sum_poses_kernel reads (entry e), and workgroup 0 writes the
//     (pose -> moved view) lists of that kernel, which follows in the stream.
#include <hip/hip_runtime.h>
#include <float.h>
#include <cstdlib>

#include "ecc_layout.h"
#include "ecc_pairs_device.h"

namespace {

constexpr int POSES_LANES = 8;  // lanes per fit: k01_kernel<8>'s

// WPP: waves per pair (1, 2, 4); REF: ECC_SAMPLING_REFERENCE with reference_split = 4 (one pair per workgroup).
// 256 threads, all of them members of the fit (a run-time member flag, as workgroups of more threads need, makes the compiler
// spend 161 vector registers on k01_fit_block instead of 75); the fit's slots beyond the workgroup's pairs are dead.
template <bool DERIV, int WPP, bool REF>
__global__ __launch_bounds__(256) void small_poses_kernel(EccPairParams p, EccSmallEval x, EccSmallPoses y)
{
    constexpr int PPW = REF ? 1 : 4 / WPP;  // pairs per workgroup
    static_assert(PPW <= 64 / POSES_LANES, "phase A makes 64 / POSES_LANES records per workgroup");
    extern __shared__ float stage_all[];  // WPP > 1: PPW * x.stage_stride floats
    __shared__ K01Shared<POSES_LANES> ks;
    __shared__ int4 idx_lds[PPW];  // the index tuples (P0, P1, dtr0, dtr1) of the workgroup's entries
    __shared__ double part[1][4];

    // the lists sum_poses_kernel reads (layout: ecc_poses.hip): pose k < Q has the one column k, the poses behind move nothing
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x <= y.n_poses) y.lists_d[threadIdx.x] = min((int)threadIdx.x, y.Q);
        if ((int)threadIdx.x < y.Q) y.lists_d[y.n_poses + 1 + threadIdx.x] = y.view;
    }
    // ---- phase A: records of this workgroup's entries ----
    const long long blk_first = (long long)blockIdx.x * PPW;
    if (threadIdx.x < PPW && blk_first + threadIdx.x < p.count) {
        const int e = (int)(blk_first + threadIdx.x), u = e / y.Q, q = e - u * y.Q, v = y.view, pv = p.n_views + q;
        int4 t = make_int4(0, 0, 0, 0);
        if (u != v) t = u < v ? make_int4(u, pv, u, v) : make_int4(pv, u, v, u);
        idx_lds[threadIdx.x] = t;
    }
    __syncthreads();
    // the patch list is read in place, from the kernel-argument segment (small_eval_kernel.hip); magic: the two views of the
    // same argument must agree, or every value of the launch is NaN
    typedef const char __attribute__((address_space(4))) * KernargBytes;
    static_assert(alignof(EccSmallEval) == 8 && alignof(EccPairParams) == 8, "layout of the kernel arguments");
    const EccSmallEvalArg xs = (EccSmallEvalArg)((KernargBytes)__builtin_amdgcn_kernarg_segment_ptr() + ((sizeof(EccPairParams) + 7) & ~(size_t)7));
    const bool args_ok = xs->magic == ECC_SMALL_MAGIC && x.magic == ECC_SMALL_MAGIC && xs->patch_count == x.patch_count;
    k01_fit_block<POSES_LANES>(p, blk_first, PPW, ks, xs, reinterpret_cast<const int32_t*>(idx_lds));  // ends with a barrier

    // ---- phase B ----
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // wave-uniform (slot: a scalar, and with it the record's address)
    const int slot = REF ? 0 : __builtin_amdgcn_readfirstlane(wave / WPP), sub = REF ? wave : wave % WPP;
    const long long local = blk_first + slot;
    const bool live = local < p.count;
    const EccPairRecord* rec = &ks.recs[slot];
    double acc = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
    if (REF) {  // pairs_reference_kernel<false, 4>: thread T takes k = T, T + 256, ..., the wave sums are added in wave order
        if (live) {
            float K0[8], K1[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                K0[i] = uniformf(rec->K0[i]);
                K1[i] = uniformf(rec->K1[i]);
            }
            const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
            reference_loop<false>(p, K0, K1, (GlobalFloats)p.slabs[iD0], (GlobalFloats)p.slabs[iD1], (int)threadIdx.x, 256, acc, m2, m3, m4);
        }
        ecc_sum::wave_sum(acc);
        if (lane == 0) put_wave_partials<false>(part, wave, acc, m2, m3, m4);
        __syncthreads();
        add_wave_partials<false>(part, acc, m2, m3, m4);
    } else {
        float* stage = WPP > 1 ? stage_all + (size_t)slot * x.stage_stride : nullptr;
        if (live) {
            const int iD0 = __builtin_amdgcn_readfirstlane(rec->iD0), iD1 = __builtin_amdgcn_readfirstlane(rec->iD1);
            pair_accumulate<DERIV, false, WPP>(p, rec, iD0, iD1, lane, acc, m2, m3, m4, sub, stage);
        }
        if (WPP > 1) {
            __syncthreads();  // every wave of the pair has stored its trips
            if (live && sub == 0) resum_staged<false>(p, uniformf(rec->K1[6]), uniformf(rec->K1[7]), lane, 64, stage, 0, acc, m2, m3, m4);
        }
        ecc_sum::wave_sum(acc);
    }

    // ---- phase C: the value of entry `local`, where sum_poses_kernel looks for it ----
    if (live && sub == 0 && lane == 0) p.pair_values[local] = args_ok ? (float)acc : __int_as_float(0x7fc00000);
}

}  // namespace

// Host-side plan of the launch: waves per pair by launch size, LDS for the staged terms.  Returns 0 when the metric's state is
// one this launch does not take (include/ecc_hip.h lists them next to ecc_metric_evaluate_gradient); the caller then goes
// through the pose batch.
extern "C" int ecc_small_poses_plan(const EccPairParams* p, int Q, int* wpp, size_t* lds_bytes)
{
    if (Q < 1 || Q > ECC_SMALL_PATCH_MAX || p->n_views < 2 || p->use_corr || p->K01_out) return 0;
    const size_t bytes = sizeof(float) * (size_t)((p->k_limit + 63) & ~63);
    if (p->reference_arithmetic) {
        if (p->reference_split != 4) return 0;
        *wpp = 4;
        *lds_bytes = 0;
        return 1;
    }
    // ecc_launch_pairs' thresholds; a user-chosen dkappa with tens of thousands of samples per pair: no stage, one wave per pair
    const long long entries = (long long)p->n_views * Q;
    int w = entries <= ECC_PAIRS_SPLIT4_MAX ? 4 : (entries <= ECC_PAIRS_SPLIT_MAX ? 2 : 1);
    if ((size_t)(4 / w) * bytes > 40 * 1024) w = 1;
    *wpp = w;
    *lds_bytes = w > 1 ? (size_t)(4 / w) * bytes : 0;
    return 1;
}

// p: the launch as fill_pair_params left it for an all-pairs evaluation, PinvTs / Cs the metric's device arrays, pair_values the
// n_views * Q slots; x: the patch list (entry q: E1 of probe q, view n_views + q); y: the moved view and the lists' address.
extern "C" hipError_t ecc_launch_small_poses(const EccPairParams* p, const EccSmallEval* x, const EccSmallPoses* y, hipStream_t stream)
{
    int wpp = 0;
    size_t lds = 0;
    if (!ecc_small_poses_plan(p, y->Q, &wpp, &lds) || x->patch_count != y->Q || y->n_poses < y->Q || y->n_poses >= 256 ||
        y->view < 0 || y->view >= p->n_views || !p->pair_values || !y->lists_d)
        return hipErrorInvalidValue;
    EccPairParams pp = *p;
    pp.indices = nullptr;  // the tuples are made in the kernel
    pp.records = nullptr;  // the records stay in LDS
    pp.record_slots = pp.value_slots = nullptr;
    pp.cost = nullptr;
    pp.patch_count = 0;
    pp.skip_enabled = 0;
    pp.first = 0;
    pp.count = (long long)p->n_views * y->Q;
    EccSmallEval xx = *x;
    xx.stage_stride = (p->k_limit + 63) & ~63;
    xx.magic = ECC_SMALL_MAGIC;
    xx.done_out = nullptr;
    const int ppw = p->reference_arithmetic ? 1 : 4 / wpp;
    const dim3 grid((unsigned)((pp.count + ppw - 1) / ppw)), block(256);
#define ECC_POSES(D, W, R) hipLaunchKernelGGL((small_poses_kernel<D, W, R>), grid, block, lds, stream, pp, xx, *y)
    if (p->reference_arithmetic) ECC_POSES(true, 4, true);  // (the reference arithmetic takes is_derivative at run time)
    else if (p->is_derivative) {
        if (wpp == 4) ECC_POSES(true, 4, false);
        else if (wpp == 2) ECC_POSES(true, 2, false);
        else ECC_POSES(true, 1, false);
    } else {
        if (wpp == 4) ECC_POSES(false, 4, false);
        else if (wpp == 2) ECC_POSES(false, 2, false);
        else ECC_POSES(false, 1, false);
    }
#undef ECC_POSES
    return hipGetLastError();
}
