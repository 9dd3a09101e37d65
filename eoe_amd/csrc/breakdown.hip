// The per-class breakdown of an evaluation's scores on the device: which class causes the misses.  A sample's side is 0 (nominal)
// or 1 (anomalous) by its class (`data.ad_targets`); the sub-problem of class k is class k against the pool of ALL samples of the
// other side, label 1 on the anomalous side.  Per class: 2U (the ROC AUC's integer numerator), the count of false positives at the
// threshold where the sub-problem's TPR first reaches a level, that threshold, and -- for an anomalous class -- the average
// precision.  Row K is the pooled problem (every anomalous sample against every nominal one): its threshold and counts.  The rates
// are one division each and stay with the caller (host, fp64).  Exact integers, no sort, no atomics; the one floating-point sum (AP)
// has a fixed order.
//
//   count pass    thread i walks all j through 256-wide LDS tiles as curve_count_kernel (curves.hip) does; a tile entry is the score
//                 and one packed word (dense class id, side << 16), both read as LDS broadcasts.  Counts, all in registers:
//                     gt_all, ge_all   #{j: s_j > s_i}, #{j: s_j >= s_i}            gt_s1, ge_s1   the same over the anomalous side
//                     gt_own, ge_own   the same over i's own class                  eqb_own, eqb_s1   #{j < i: s_j == s_i} in the
//                                                                                   own class / on the anomalous side
//                 (the nominal side is all - s1; "opposite" and "own side" are picked from the two after the loop).
//                 Thresholds: place m among the positives, descending, lies in the tie group with gt < m <= ge.  For an anomalous
//                 class the positives are the class: its member with gt_own < m[k] <= ge_own and eqb_own == 0 (the smallest index of
//                 the group, whose bits a reversed stable sort keeps: -0.0 against 0.0) writes thr[k], fps[k] = ge_s0 and tps[k] =
//                 ge_own.  For the pooled problem and for every nominal class the positives are the whole anomalous side: the one
//                 sample with gt_s1 < m_pooled <= ge_s1 and eqb_s1 == 0 writes row K.  One writer per slot.
//                 Per sample it leaves ge_opp + gt_opp, ge_own and ge_opp for the reduce pass.
//   reduce pass   workgroup k walks the n samples in index order in chunks of 256 and sums over the members of class k
//                     S = sum (ge_opp + gt_opp)        int64        2U = S for a nominal class, 2 n_k n_opp - S for an anomalous one
//                     #{b in k: s_b >= thr[K]}         int64        (nominal classes: their false positives at the pooled threshold)
//                     sum ge_own / (ge_own + ge_opp)   fp64         (anomalous classes; divided by n_k here)
//                 per-thread partials in index order, then a fixed tree over the 256 threads.  It reads the thresholds the count
//                 pass wrote, on the same stream; nothing comes back to the host in between.
// Two memsets (the integer table, the thresholds) and two launches, all on the caller's stream.
#include "common.h"

namespace {

constexpr int BD_NT = 256;                     // both passes: threads per workgroup = scores per LDS tile / samples per chunk
constexpr int BD_N_MAX = 1 << 20;              // the cap of curves.hip
constexpr int BD_K_MAX = 1024;                 // a dense class id fits the low 16 bits of the packed word
constexpr unsigned BD_DEAD = 0xFFFFu;          // class field of a sample whose id is outside [0, K): it is in no class and no pool
constexpr int BD_COLS = 4;                     // out_counts[k] = {2U, fps, tps, n_k}

size_t plane_bytes(int n) { return align_up((size_t)n * 4, 256); }

__device__ __forceinline__ unsigned pack_class(const int32_t* __restrict__ cls, const uint8_t* __restrict__ side, int j, int K) {
    const int c = cls[j];
    if (c < 0 || c >= K) return BD_DEAD;
    return (unsigned)c | ((side[c] ? 1u : 0u) << 16);
}

__global__ __launch_bounds__(BD_NT) void breakdown_count_kernel(const float* __restrict__ s, const int32_t* __restrict__ cls,
                                                                const uint8_t* __restrict__ side, const int32_t* __restrict__ m_cls,
                                                                int m_pooled, int n, int K, unsigned* __restrict__ p_pack,
                                                                unsigned* __restrict__ p_sum, unsigned* __restrict__ p_own,
                                                                unsigned* __restrict__ p_opp, int64_t* __restrict__ out_counts,
                                                                float* __restrict__ out_thr) {
    __shared__ float ts[BD_NT];
    __shared__ unsigned tp[BD_NT];
    const int i = blockIdx.x * BD_NT + threadIdx.x;
    const bool inside = i < n;
    const unsigned pi = inside ? pack_class(cls, side, i, K) : BD_DEAD;
    const bool live = pi != BD_DEAD;
    const float si = inside ? s[i] : 0.f;
    const unsigned ci = pi & 0xFFFFu;
    unsigned gt_all = 0, ge_all = 0, gt_s1 = 0, ge_s1 = 0, gt_own = 0, ge_own = 0, eqb_own = 0, eqb_s1 = 0;
    for (int j0 = 0; j0 < n; j0 += BD_NT) {
        const int j = j0 + threadIdx.x;
        const unsigned pj = j < n ? pack_class(cls, side, j, K) : BD_DEAD;
        // a sample without a class compares as NaN: it is counted nowhere
        ts[threadIdx.x] = (j < n && pj != BD_DEAD) ? s[j] : __uint_as_float(0x7FC00000u);
        tp[threadIdx.x] = pj;
        __syncthreads();
        const int m = n - j0 < BD_NT ? n - j0 : BD_NT;
        const int before = i - j0;                           // tile entries k < before have j < i
#pragma unroll 8
        for (int k = 0; k < m; ++k) {                        // every lane reads the same two words: LDS broadcasts
            const float sj = ts[k];
            const unsigned pk = tp[k];
            const unsigned ge = sj >= si, gt = sj > si;
            const unsigned s1 = pk >> 16;                    // 0 or 1 (the dead marker has no bit there)
            const unsigned own = (pk & 0xFFFFu) == ci;
            const unsigned eqb = (ge & ~gt & 1u) & (unsigned)(k < before);
            gt_all += gt;
            ge_all += ge;
            gt_s1 += gt & s1;
            ge_s1 += ge & s1;
            gt_own += gt & own;
            ge_own += ge & own;
            eqb_own += eqb & own;
            eqb_s1 += eqb & s1;
        }
        __syncthreads();
    }
    if (!inside) return;
    const unsigned sd = (pi >> 16) & 1u;
    const unsigned gt_s0 = gt_all - gt_s1, ge_s0 = ge_all - ge_s1;
    const unsigned gt_opp = sd ? gt_s0 : gt_s1, ge_opp = sd ? ge_s0 : ge_s1;
    p_pack[i] = pi;
    p_sum[i] = live ? ge_opp + gt_opp : 0u;
    p_own[i] = live ? ge_own : 0u;
    p_opp[i] = live ? ge_opp : 0u;
    if (!live || !sd) return;
    const int mk = m_cls[ci];                                // ci < K: the sample is live
    if (eqb_own == 0 && mk >= 1 && gt_own < (unsigned)mk && (unsigned)mk <= ge_own) {
        out_thr[ci] = si;
        out_counts[(size_t)ci * BD_COLS + 1] = (int64_t)ge_s0;
        out_counts[(size_t)ci * BD_COLS + 2] = (int64_t)ge_own;
    }
    if (eqb_s1 == 0 && m_pooled >= 1 && gt_s1 < (unsigned)m_pooled && (unsigned)m_pooled <= ge_s1) {
        out_thr[K] = si;
        out_counts[(size_t)K * BD_COLS + 1] = (int64_t)ge_s0;
        out_counts[(size_t)K * BD_COLS + 2] = (int64_t)ge_s1;
    }
}

__global__ __launch_bounds__(BD_NT) void breakdown_reduce_kernel(const float* __restrict__ s, const uint8_t* __restrict__ side, int n, int K,
                                                                 const unsigned* __restrict__ p_pack, const unsigned* __restrict__ p_sum,
                                                                 const unsigned* __restrict__ p_own, const unsigned* __restrict__ p_opp,
                                                                 int64_t* __restrict__ out_counts, double* __restrict__ out_ap,
                                                                 float* __restrict__ out_thr) {
    __shared__ long long bi[BD_NT];
    __shared__ double bd[BD_NT];
    const unsigned k = blockIdx.x;                           // < K: the grid is K workgroups
    const unsigned sd = side[k] ? 1u : 0u;
    const float t_pool = out_thr[K];                         // written by the count pass (or cleared: no anomalous sample)
    long long sum = 0, members = 0, opposite = 0, above = 0;
    double ap = 0.0;
    for (int c0 = 0; c0 < n; c0 += BD_NT) {
        const int i = c0 + (int)threadIdx.x;
        if (i >= n) break;
        const unsigned pi = p_pack[i];
        if (pi == BD_DEAD) continue;
        opposite += ((pi >> 16) & 1u) != sd;
        if ((pi & 0xFFFFu) != k) continue;
        ++members;
        sum += (long long)p_sum[i];
        if (sd) {
            const double own = (double)p_own[i];             // >= 1: the sample counts itself
            ap += own / (own + (double)p_opp[i]);
        } else {
            above += s[i] >= t_pool;
        }
    }
    sum = block_tree_sum<BD_NT>(sum, bi);
    members = block_tree_sum<BD_NT>(members, bi);
    opposite = block_tree_sum<BD_NT>(opposite, bi);
    above = block_tree_sum<BD_NT>(above, bi);
    ap = block_tree_sum<BD_NT>(ap, bd);
    if (threadIdx.x != 0) return;
    int64_t* row = out_counts + (size_t)k * BD_COLS;
    row[0] = sd ? 2 * members * opposite - sum : sum;
    row[3] = members;
    out_ap[k] = (sd && members > 0) ? ap / (double)members : 0.0;
    if (!sd) {                                               // a nominal class: the pooled positives' threshold, its own false positives
        row[1] = above;
        row[2] = out_counts[(size_t)K * BD_COLS + 2];
        out_thr[k] = t_pool;
    }
}

bool in_range(int n, int K) { return n >= 1 && n <= BD_N_MAX && K >= 1 && K <= BD_K_MAX; }

}  // namespace

extern "C" size_t eoe_class_breakdown_scratch_bytes(int n, int K) { return in_range(n, K) ? 4 * plane_bytes(n) : 0; }

extern "C" int eoe_class_breakdown(const float* scores, const int32_t* class_ids, const uint8_t* side_per_class, const int32_t* m_per_class,
                                   int m_pooled, int n, int K, int64_t* out_counts, double* out_ap, float* out_thr, void* scratch,
                                   void* stream) {
    EOE_CHECK_ARG(scores, "class_breakdown: null scores");
    EOE_CHECK_ARG(class_ids, "class_breakdown: null class_ids");
    EOE_CHECK_ARG(side_per_class, "class_breakdown: null side_per_class");
    EOE_CHECK_ARG(m_per_class, "class_breakdown: null m_per_class");
    EOE_CHECK_ARG(out_counts, "class_breakdown: null out_counts");
    EOE_CHECK_ARG(out_ap, "class_breakdown: null out_ap");
    EOE_CHECK_ARG(out_thr, "class_breakdown: null out_thr");
    EOE_CHECK_ARG(scratch, "class_breakdown: null scratch");
    EOE_CHECK_ARG(n >= 1 && n <= BD_N_MAX, "class_breakdown: n must be in [1, %d], not %d", BD_N_MAX, n);
    EOE_CHECK_ARG(K >= 1 && K <= BD_K_MAX, "class_breakdown: K must be in [1, %d], not %d", BD_K_MAX, K);
    EOE_CHECK_ARG(m_pooled >= 0 && m_pooled <= n, "class_breakdown: m_pooled must be in [0, n = %d], not %d", n, m_pooled);
    EOE_CHECK_ARG(((uintptr_t)scores & 3) == 0, "class_breakdown: scores must be 4-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)class_ids & 3) == 0, "class_breakdown: class_ids must be 4-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)m_per_class & 3) == 0, "class_breakdown: m_per_class must be 4-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)out_counts & 7) == 0, "class_breakdown: out_counts must be 8-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)out_ap & 7) == 0, "class_breakdown: out_ap must be 8-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)out_thr & 3) == 0, "class_breakdown: out_thr must be 4-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)scratch & 3) == 0, "class_breakdown: scratch must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = plane_bytes(n);
    char* base = static_cast<char*>(scratch);
    unsigned* p_pack = reinterpret_cast<unsigned*>(base);
    unsigned* p_sum = reinterpret_cast<unsigned*>(base + plane);
    unsigned* p_own = reinterpret_cast<unsigned*>(base + 2 * plane);
    unsigned* p_opp = reinterpret_cast<unsigned*>(base + 3 * plane);
    ProfScope ps("class_breakdown", 10.0 * (double)n * (double)n, 24.0 * (double)n + 4.0 * (double)n * (double)K, stream);
    // a slot without a writer (a class id nobody carries, a side without samples) reads as 0
    hipError_t e = hipMemsetAsync(out_counts, 0, (size_t)(K + 1) * BD_COLS * sizeof(int64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(out_thr, 0, (size_t)(K + 1) * sizeof(float), st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "class_breakdown: clearing the outputs: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(breakdown_count_kernel, dim3(cdiv(n, BD_NT)), dim3(BD_NT), 0, st, scores, class_ids, side_per_class, m_per_class,
                       m_pooled, n, K, p_pack, p_sum, p_own, p_opp, out_counts, out_thr);
    EOE_CHECK_LAUNCH("class_breakdown (count)");
    hipLaunchKernelGGL(breakdown_reduce_kernel, dim3(K), dim3(BD_NT), 0, st, scores, side_per_class, n, K, (const unsigned*)p_pack,
                       (const unsigned*)p_sum, (const unsigned*)p_own, (const unsigned*)p_opp, out_counts, out_ap, out_thr);
    EOE_CHECK_LAUNCH("class_breakdown (reduce)");
    return 0;
}
