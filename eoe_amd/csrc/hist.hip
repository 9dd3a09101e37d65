// Anomaly-score histograms on the device (`ad_trainer.py:458-465, 541-546`: `SummaryWriter.add_histogram` on host copies of an epoch's
// scores, one picture per label group).  What TensorBoard stores is `np.histogram(values, bins=edges)` over a fixed table of edges plus
// five scalars; this file makes the untrimmed integer counts and the scalars of BOTH label groups in one pass over the scores.  The
// trimming to the occupied range is a few integer operations on the counts and stays with the caller (eoe_amd/metrics.py).
//
//   bucket        b = #{edges <= v} - 1 by a binary search in float64 over the table held in LDS (an upload of the host's table: never
//                 a pow or log here, which would move edges by an ulp); bin b = [e_b, e_b+1), v == the last edge belongs to the last
//                 bin, a v outside [e_0, e_E-1] to none.  IEEE compares: -0.0 is 0.0.
//   counts        per workgroup a table of 2 x (E - 1) 32-bit counters in LDS, filled by LDS integer atomics, its non-zero entries
//                 folded into the global table by integer atomic adds (cleared by a memset on the stream beforehand): integers,
//                 the same on every run.
//   scalars       count / min / max / sum / sum of squares per group in float64 without a floating-point atomic: thread -> wave
//                 butterfly -> the 4 waves in order -> one partial row per workgroup in scratch; a second launch of one workgroup
//                 reduces the rows the same way.  The grid is a function of n alone, so every step has a fixed order and two runs
//                 give the same bits.  The first launch writes every partial row the second reads: scratch may arrive dirty.
// A memset and two launches, all on the caller's stream.
#include "common.h"

namespace {

constexpr int HS_NT = 256;                     // threads per workgroup; also the most workgroups (the finish kernel has one thread per partial row)
constexpr int HS_WAVES = HS_NT / 64;
constexpr int HS_MAX_EDGES = 4001;             // 4 000 bins: 8 E + 2 * 4 (E - 1) bytes of LDS and the reduction's 400 stay under 64 KB
constexpr int HS_Q = 10;                       // 2 groups x (count, min, max, sum, sum of squares)

int hist_grid(int n) { return n < HS_NT * HS_NT ? cdiv(n, HS_NT) : HS_NT; }

enum { RED_SUM = 0, RED_MIN = 1, RED_MAX = 2 };
__host__ __device__ constexpr int red_kind(int q) { return q % 5 == 1 ? RED_MIN : (q % 5 == 2 ? RED_MAX : RED_SUM); }
__device__ __forceinline__ double red_identity(int kind) {
    return kind == RED_MIN ? __builtin_huge_val() : (kind == RED_MAX ? -__builtin_huge_val() : 0.0);
}
__device__ __forceinline__ double red_op(double a, double b, int kind) { return kind == RED_MIN ? fmin(a, b) : (kind == RED_MAX ? fmax(a, b) : a + b); }

// the workgroup's HS_Q values from one value per thread each: a butterfly within the wave (every lane ends with the same bits), the
// waves' results through LDS, combined in wave order by thread q.  Valid in threads q < HS_Q.
__device__ __forceinline__ double block_reduce(double (&v)[HS_Q], double (*red)[HS_Q]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < HS_Q; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[q] = red_op(v[q], __shfl_xor(v[q], o, 64), red_kind(q));
        if (lane == 0) red[wave][q] = v[q];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < HS_Q) {
        const int kind = red_kind((int)threadIdx.x);
        r = red[0][threadIdx.x];
        for (int w = 1; w < HS_WAVES; ++w) r = red_op(r, red[w][threadIdx.x], kind);
    }
    return r;
}

__global__ __launch_bounds__(HS_NT) void score_hist_kernel(const float* __restrict__ s, const int64_t* __restrict__ labels, int n,
                                                           const double* __restrict__ edges, int E, int* __restrict__ counts,
                                                           double* __restrict__ part) {
    extern __shared__ double hs_lds[];                       // edges [E], then counters [2][E - 1]
    __shared__ double red[HS_WAVES][HS_Q];
    double* se = hs_lds;
    unsigned* sc = reinterpret_cast<unsigned*>(hs_lds + E);
    const int nb = E - 1;
    for (int i = threadIdx.x; i < E; i += HS_NT) se[i] = edges[i];
    for (int i = threadIdx.x; i < 2 * nb; i += HS_NT) sc[i] = 0u;
    __syncthreads();
    double v[HS_Q];
#pragma unroll
    for (int q = 0; q < HS_Q; ++q) v[q] = red_identity(red_kind(q));
    const int64_t stride = (int64_t)gridDim.x * HS_NT;
    for (int64_t i = (int64_t)blockIdx.x * HS_NT + threadIdx.x; i < n; i += stride) {
        int g = 0;
        if (labels) {
            const int64_t y = labels[i];
            g = y == 0 ? 0 : (y == 1 ? 1 : -1);
        }
        if (g < 0) continue;                                 // any other label, e.g. -1 for unlabelled images, is in neither group
        const double x = (double)s[i];
        int lo = 0, hi = E;                                  // lo -> #{edges <= x}
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (se[mid] <= x) lo = mid + 1; else hi = mid;
        }
        int b = lo - 1;
        if (b == nb && x == se[nb]) b = nb - 1;              // the last bin is closed on both sides
        if (b >= 0 && b < nb) atomicAdd(&sc[g * nb + b], 1u);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (g == k) {
                v[5 * k + 0] += 1.0;
                v[5 * k + 1] = fmin(v[5 * k + 1], x);
                v[5 * k + 2] = fmax(v[5 * k + 2], x);
                v[5 * k + 3] += x;
                v[5 * k + 4] += x * x;                       // exact product of two floats; only the sum rounds
            }
        }
    }
    const double r = block_reduce(v, red);                   // its barrier also ends the LDS atomics above
    if (threadIdx.x < HS_Q) part[(size_t)blockIdx.x * HS_Q + threadIdx.x] = r;
    for (int i = threadIdx.x; i < 2 * nb; i += HS_NT) {
        const unsigned c = sc[i];
        if (c) atomicAdd(&counts[i], (int)c);
    }
}

// one workgroup: thread t holds partial row t (t < rows <= HS_NT).  An empty group reports count 0 and zeros for the rest.
__global__ __launch_bounds__(HS_NT) void score_hist_finish_kernel(const double* __restrict__ part, int rows, double* __restrict__ stats) {
    __shared__ double red[HS_WAVES][HS_Q];
    __shared__ double res[HS_Q];
    double v[HS_Q];
#pragma unroll
    for (int q = 0; q < HS_Q; ++q) v[q] = (int)threadIdx.x < rows ? part[(size_t)threadIdx.x * HS_Q + q] : red_identity(red_kind(q));
    const double r = block_reduce(v, red);
    if (threadIdx.x < HS_Q) res[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x < HS_Q) stats[threadIdx.x] = res[threadIdx.x / 5 * 5] > 0.0 ? r : 0.0;
}

}  // namespace

extern "C" size_t eoe_score_hist_scratch_bytes(int n) { return n > 0 ? (size_t)hist_grid(n) * HS_Q * sizeof(double) : 0; }

extern "C" int eoe_score_hist(const float* scores, const int64_t* labels, int n, const double* edges_host, const double* edges, int E,
                              int32_t* out_counts, double* out_stats, void* scratch, void* stream) {
    EOE_CHECK_ARG(scores && edges_host && edges && out_counts && out_stats && scratch, "score_hist: null scores, edges, output or scratch");
    EOE_CHECK_ARG(n >= 1, "score_hist: n must be at least 1, not %d", n);
    EOE_CHECK_ARG(E >= 2 && E <= HS_MAX_EDGES, "score_hist: E must be in [2, %d], not %d", HS_MAX_EDGES, E);
    for (int i = 0; i < E; ++i)
        EOE_CHECK_ARG(edges_host[i] - edges_host[i] == 0.0 && (i == 0 || edges_host[i] > edges_host[i - 1]),
                      "score_hist: edges must be finite and strictly ascending (edge %d)", i);
    EOE_CHECK_ARG(((uintptr_t)scratch & 7) == 0 && ((uintptr_t)out_stats & 7) == 0 && ((uintptr_t)out_counts & 3) == 0,
                  "score_hist: scratch and out_stats must be 8-byte aligned, out_counts 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nb = E - 1, grid = hist_grid(n);
    double* part = static_cast<double*>(scratch);
    ProfScope ps("score_hist", 0.0, (labels ? 12.0 : 4.0) * (double)n, stream);
    hipError_t e = hipMemsetAsync(out_counts, 0, (size_t)2 * nb * sizeof(int32_t), st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "score_hist: clearing the counts: %s", hipGetErrorString(e));
    const size_t lds = (size_t)E * sizeof(double) + (size_t)2 * nb * sizeof(unsigned);
    hipLaunchKernelGGL(score_hist_kernel, dim3(grid), dim3(HS_NT), lds, st, scores, labels, n, edges, E, out_counts, part);
    EOE_CHECK_LAUNCH("score_hist (count)");
    hipLaunchKernelGGL(score_hist_finish_kernel, dim3(1), dim3(HS_NT), 0, st, (const double*)part, grid, out_stats);
    EOE_CHECK_LAUNCH("score_hist (finish)");
    return 0;
}
