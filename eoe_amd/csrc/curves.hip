// ROC and precision-recall curves on the device (`ad_trainer.py:452-455, 516-522`: sklearn's `roc_curve` and
// `precision_recall_curve` on host copies of the labels and scores).  What both curves are made of is the table
//     (fps_k, tps_k, thr_k),  k < K,  thr_0 > thr_1 > ... the K distinct scores,
//     tps_k = #{j positive: s_j >= thr_k},   fps_k = #{j: s_j >= thr_k} - tps_k
// and, for the ROC, the same table without the points that lie on a straight line between their neighbours
// (`drop_intermediate`).  The rates are one division each and stay with the caller (host, fp64).  Everything here is exact in
// integers; no sort, no atomics, no floating-point sum.
//
//   count pass    thread i walks all j through 256-wide LDS tiles, as rank_pairs_kernel (elementwise.hip) does, and counts
//                     gt_all = #{j: s_j > s_i}   ge_all = #{j: s_j >= s_i}   ge_pos = #{j positive: s_j >= s_i}
//                     eq_before = #{j < i: s_j == s_i}
//                 Element i stands for its group of equal scores iff eq_before == 0 (the smallest index of the group: the element
//                 a reversed stable sort leaves last in the group, so the threshold has that element's bits, -0.0 against 0.0
//                 included).  gt_all is the group's first place among the n descending places and differs between groups: the
//                 representative stores (fps, tps, thr) and a flag at place gt_all.  n^2 compares, cdiv(n, 256) workgroups.
//   compaction    one workgroup of 1 024 threads walks the n places in chunks of 1 024: an exclusive prefix sum of the chunk's
//                 flags in LDS plus the carry of the chunks before it is a flagged place's slot.  K = the final carry.
//   ROC points    the same walk over the K slots of the table just written (K is read on the device, nothing comes back to the
//                 host in between), the flag computed on the fly: slot 0, slot K-1 and every slot whose second difference of fps
//                 or of tps is not 0; every slot when K <= 2 or drop_intermediate is off.
// Three launches and one memset of the flags, all on the caller's stream.
#include "common.h"

namespace {

constexpr int CV_NT = 256;                     // count pass: threads per workgroup = scores per LDS tile
constexpr int CV_SCAN = 1024;                  // compaction: places per chunk = threads of its one workgroup
constexpr int CV_N_MAX = 1 << 20;

size_t plane_bytes(int n) { return align_up((size_t)n * 4, 256); }

__global__ __launch_bounds__(CV_NT) void curve_count_kernel(const float* __restrict__ s, const int64_t* __restrict__ labels, int64_t positive,
                                                            int n, int* __restrict__ flag, int* __restrict__ p_fps,
                                                            int* __restrict__ p_tps, float* __restrict__ p_thr) {
    __shared__ float ts[CV_NT];
    __shared__ int tp[CV_NT];
    const int i = blockIdx.x * CV_NT + threadIdx.x;
    const bool live = i < n;
    const float si = live ? s[i] : 0.f;
    unsigned gt_all = 0, ge_all = 0, ge_pos = 0, eq_before = 0;
    for (int j0 = 0; j0 < n; j0 += CV_NT) {
        const int j = j0 + threadIdx.x;
        ts[threadIdx.x] = j < n ? s[j] : 0.f;
        tp[threadIdx.x] = j < n ? (labels[j] == positive ? 1 : 0) : 0;
        __syncthreads();
        const int m = n - j0 < CV_NT ? n - j0 : CV_NT;
        const int before = i - j0;                           // tile entries k < before have j < i
#pragma unroll 8
        for (int k = 0; k < m; ++k) {                        // every lane reads the same word: an LDS broadcast
            const float sj = ts[k];
            const unsigned ge = sj >= si, gt = sj > si;
            gt_all += gt;
            ge_all += ge;
            ge_pos += ge & (unsigned)tp[k];
            eq_before += (ge & ~gt & 1u) & (unsigned)(k < before);
        }
        __syncthreads();
    }
    if (live && eq_before == 0 && gt_all < (unsigned)n) {    // gt_all <= n - 1 for any input (j = i is never counted)
        flag[gt_all] = 1;
        p_fps[gt_all] = (int)(ge_all - ge_pos);
        p_tps[gt_all] = (int)ge_pos;
        p_thr[gt_all] = si;
    }
}

// exclusive prefix sum of one 0 / 1 value per thread over the 1 024 threads of the workgroup; `total` = the sum.  Ballots within
// a wave, the 16 wave totals through LDS.
__device__ __forceinline__ int block_excl_scan(int f, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CV_SCAN / 64; ++w) {
        const int t = wave_tot[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();                                         // wave_tot is written again by the next chunk
    total = all;
    return before + in_wave;
}

// ROC == false: flags and records by place (count pass) -> the table, counts[0] = K.
// ROC == true:  the table's K = counts[0] slots -> the ROC table, counts[1] = K_roc.
template <bool ROC>
__global__ __launch_bounds__(CV_SCAN) void curve_compact_kernel(const int* __restrict__ flag, const int* __restrict__ p_fps,
                                                                const int* __restrict__ p_tps, const float* __restrict__ p_thr,
                                                                const int64_t* __restrict__ t_fps, const int64_t* __restrict__ t_tps,
                                                                const float* __restrict__ t_thr, int n, int drop,
                                                                int64_t* __restrict__ o_fps, int64_t* __restrict__ o_tps,
                                                                float* __restrict__ o_thr, int* __restrict__ counts) {
    __shared__ int wave_tot[CV_SCAN / 64];
    int len = n;
    if (ROC) {
        len = counts[0];
        len = len < 0 ? 0 : (len > n ? n : len);             // K <= n by construction; never trust a length read from memory
    }
    const bool all = ROC && (!drop || len <= 2);
    int carry = 0;
    for (int c0 = 0; c0 < len; c0 += CV_SCAN) {
        const int p = c0 + (int)threadIdx.x;
        int f = 0;
        if (p < len) {
            if (!ROC) f = flag[p];
            else if (all || p == 0 || p == len - 1) f = 1;
            else f = (t_fps[p - 1] - 2 * t_fps[p] + t_fps[p + 1] != 0) || (t_tps[p - 1] - 2 * t_tps[p] + t_tps[p + 1] != 0);
        }
        int total;
        const int slot = carry + block_excl_scan(f, wave_tot, total);
        if (f && slot < n) {                                 // slot <= p < n
            o_fps[slot] = ROC ? t_fps[p] : (int64_t)p_fps[p];
            o_tps[slot] = ROC ? t_tps[p] : (int64_t)p_tps[p];
            o_thr[slot] = ROC ? t_thr[p] : p_thr[p];
        }
        carry += total;
    }
    if (threadIdx.x == 0) counts[ROC ? 1 : 0] = carry;
}

}  // namespace

extern "C" size_t eoe_rank_curves_scratch_bytes(int n) { return (n > 0 && n <= CV_N_MAX) ? 4 * plane_bytes(n) : 0; }

extern "C" int eoe_rank_curves(const float* scores, const int64_t* labels, int64_t positive_label, int n, int drop_intermediate,
                               int64_t* out_fps, int64_t* out_tps, float* out_thr, int64_t* out_roc_fps, int64_t* out_roc_tps,
                               float* out_roc_thr, int32_t* out_counts, void* scratch, void* stream) {
    EOE_CHECK_ARG(scores && labels && out_fps && out_tps && out_thr && out_roc_fps && out_roc_tps && out_roc_thr && out_counts && scratch,
                  "rank_curves: null scores, labels, output or scratch");
    EOE_CHECK_ARG(n > 0 && n <= CV_N_MAX, "rank_curves: n must be in [1, %d], not %d", CV_N_MAX, n);
    EOE_CHECK_ARG(((uintptr_t)scratch & 3) == 0, "rank_curves: scratch must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = plane_bytes(n);
    char* base = static_cast<char*>(scratch);
    int* flag = reinterpret_cast<int*>(base);
    int* p_fps = reinterpret_cast<int*>(base + plane);
    int* p_tps = reinterpret_cast<int*>(base + 2 * plane);
    float* p_thr = reinterpret_cast<float*>(base + 3 * plane);
    ProfScope ps("rank_curves", 4.0 * (double)n * (double)n, 12.0 * (double)n + 2.0 * 20.0 * (double)n, stream);
    hipError_t e = hipMemsetAsync(flag, 0, (size_t)n * sizeof(int), st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "rank_curves: clearing the flags: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(curve_count_kernel, dim3(cdiv(n, CV_NT)), dim3(CV_NT), 0, st, scores, labels, positive_label, n, flag, p_fps, p_tps,
                       p_thr);
    EOE_CHECK_LAUNCH("rank_curves (count)");
    hipLaunchKernelGGL(curve_compact_kernel<false>, dim3(1), dim3(CV_SCAN), 0, st, (const int*)flag, (const int*)p_fps, (const int*)p_tps,
                       (const float*)p_thr, (const int64_t*)nullptr, (const int64_t*)nullptr, (const float*)nullptr, n, 0, out_fps, out_tps,
                       out_thr, out_counts);
    EOE_CHECK_LAUNCH("rank_curves (compact)");
    hipLaunchKernelGGL(curve_compact_kernel<true>, dim3(1), dim3(CV_SCAN), 0, st, (const int*)nullptr, (const int*)nullptr,
                       (const int*)nullptr, (const float*)nullptr, (const int64_t*)out_fps, (const int64_t*)out_tps, (const float*)out_thr, n,
                       drop_intermediate ? 1 : 0, out_roc_fps, out_roc_tps, out_roc_thr, out_counts);
    EOE_CHECK_LAUNCH("rank_curves (roc points)");
    return 0;
}
