// DeLong's estimator of the covariance of K ROC AUCs measured on the same n samples (DeLong, DeLong & Clarke-Pearson 1988), as the
// exact integer sums it is made of.  Positives are the samples with label 1 (m of them), negatives those with label 0 (n0); every
// other label is in neither.  Per column k (one model's scores) and per sample, the doubled count of the opposite side it beats or ties:
//     a[k,i] = 2 #{j negative: s_k[i] > s_k[j]} + #{j negative: s_k[i] == s_k[j]}       positive i, in [0, 2 n0]
//     b[k,j] = 2 #{i positive: s_k[i] > s_k[j]} + #{i positive: s_k[i] == s_k[j]}       negative j, in [0, 2 m]
// and from them T[k] = sum_i a[k,i] = sum_j b[k,j] (both sums are written: their equality is the caller's check), A[k,l] = sum_i
// a[k,i] a[l,i] and B[k,l] = sum_j b[k,j] b[l,j] for k <= l.  The divisions that turn these into AUCs and covariances are the caller's.
// Integer compares and integer adds only, so two runs give the same bytes; the only atomics are integer adds.
//
//   partition pass   ONE workgroup of 1 024 threads: thread t counts the positives and the negatives of its contiguous chunk of the
//                    labels, a scan over the 1 024 pairs gives its offsets, and it writes the chunk's positions into `order`:
//                    positives at [0, m), negatives at [m, m + n0), each ascending.  It leaves m, n0 and a cleared NaN counter in
//                    the table, where the next two passes read them: nothing comes back to the host in between.
//   count pass       the m x n0 comparisons of a column, once for the positives' counts and once for the negatives'.  Rows are laid
//                    out in blocks of 256: cdiv(m, 256) blocks of positives, then cdiv(n0, 256) of negatives; one row per lane.  A
//                    workgroup is (row block, slice of the opposite side, column): it walks its slice in 256-score LDS tiles -- the
//                    scores gathered through `order`, the tail padded with NaN, which compares false -- reads them back as 16-byte
//                    LDS broadcasts and keeps `greater` and `equal` in registers.  A block of negatives negates its own and the
//                    tile's scores, so that the one loop `x > y` counts the positives ABOVE a negative (-0.0 == 0.0 and the
//                    infinities survive the sign flip).  The opposite side is cut into `slices` so that a few row blocks still fill
//                    the chip (10 000 scores are 40 row blocks); each slice adds its 2 gt + eq to the row's counter with one integer
//                    atomic.  Slice 0 counts the NaN scores of its rows into the table.
//   reduce pass      workgroup (pair k <= l, side): the 256 threads walk the side's rows with stride 256, sum a_k a_l (and a_k when
//                    k == l) in int64, then a fixed tree over the threads.
// One memset (the row counters) and three launches, all on the caller's stream.
//
// Ranges: a row counter is at most 2 max(m, n0) <= 2^21 (uint32).  A[k,l] <= m (2 n0)^2 and B[k,l] <= n0 (2 m)^2 with m + n0 <= n, at
// most 16 n^3 / 27: 4.4e14 at n = 90 000 and 6.9e17 < 2^63 = 9.2e18 at the cap n = 2^20.  T <= 2 m n0 <= n^2 / 2 < 2^40.
#include "common.h"

namespace {

constexpr int DL_NT = 256;                     // count and reduce pass: threads per workgroup = rows per block = scores per LDS tile
constexpr int DL_PART_NT = 1024;               // partition pass: one workgroup
constexpr int DL_N_MAX = 1 << 20;              // the cap of breakdown.hip
constexpr int DL_K_MAX = 8;
constexpr int DL_TARGET_WGS = 2048;            // count pass: slices are added until the grid has about this many workgroups ...
constexpr int DL_MAX_SLICES = 64;              // ... but never more than this

size_t order_bytes(int n) { return align_up((size_t)n * 4, 256); }
int row_blocks(int n) { return cdiv(n, DL_NT) + 1; }                // cdiv(m, 256) + cdiv(n0, 256) <= cdiv(n, 256) + 1
int pairs(int K) { return K * (K + 1) / 2; }
int slices_for(int n, int K) {
    const int s = cdiv(DL_TARGET_WGS, row_blocks(n) * K);
    return s < 1 ? 1 : (s > DL_MAX_SLICES ? DL_MAX_SLICES : s);
}

__global__ __launch_bounds__(DL_PART_NT) void delong_partition_kernel(const int64_t* __restrict__ labels, int n, int* __restrict__ order,
                                                                      int64_t* __restrict__ out_sizes) {
    __shared__ int sp[2][DL_PART_NT];
    __shared__ int sq[2][DL_PART_NT];
    const int t = threadIdx.x;
    const int chunk = (n + DL_PART_NT - 1) / DL_PART_NT;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int p = 0, q = 0;
    for (int i = lo; i < hi; ++i) {
        const int64_t y = labels[i];
        p += y == 1;
        q += y == 0;
    }
    // inclusive scan of the 1 024 (p, q) pairs, double-buffered
    int cur = 0;
    sp[0][t] = p;
    sq[0][t] = q;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < DL_PART_NT; d <<= 1) {
        const int vp = sp[cur][t] + (t >= d ? sp[cur][t - d] : 0);
        const int vq = sq[cur][t] + (t >= d ? sq[cur][t - d] : 0);
        sp[cur ^ 1][t] = vp;
        sq[cur ^ 1][t] = vq;
        cur ^= 1;
        __syncthreads();
    }
    const int m = sp[cur][DL_PART_NT - 1], n0 = sq[cur][DL_PART_NT - 1];
    int at_p = sp[cur][t] - p, at_q = m + sq[cur][t] - q;              // < m and < m + n0 <= n while there is something to write
    for (int i = lo; i < hi; ++i) {
        const int64_t y = labels[i];
        if (y == 1) order[at_p++] = i;
        else if (y == 0) order[at_q++] = i;
    }
    if (t == 0) {
        out_sizes[0] = m;
        out_sizes[1] = n0;
        out_sizes[2] = 0;                                              // the NaN counter of the count pass
    }
}

__global__ __launch_bounds__(DL_NT) void delong_count_kernel(const float* __restrict__ scores, const int* __restrict__ order, int n,
                                                             int slices, int rows_cap, unsigned* __restrict__ cnt,
                                                             int64_t* __restrict__ out_sizes) {
    __shared__ __attribute__((aligned(16))) float ts[DL_NT];
    const int m = (int)out_sizes[0], n0 = (int)out_sizes[1];          // written by the partition pass: m + n0 <= n
    const int pb = (m + DL_NT - 1) / DL_NT, nb = (n0 + DL_NT - 1) / DL_NT;
    const int b = blockIdx.x;
    if (b >= pb + nb) return;                                          // the grid is sized for the worst split of n
    const bool pos = b < pb;
    const int own_n = pos ? m : n0, own_at = pos ? 0 : m;
    const int opp_n = pos ? n0 : m, opp_at = pos ? m : 0;
    const float sign = pos ? 1.f : -1.f;
    const float* __restrict__ s = scores + (size_t)blockIdx.z * n;
    const int r = (pos ? b : b - pb) * DL_NT + (int)threadIdx.x;      // the row within its side
    const bool inside = r < own_n;
    const float x = inside ? sign * s[order[own_at + r]] : __uint_as_float(0x7FC00000u);
    if (blockIdx.y == 0 && inside && x != x) atomicAdd(reinterpret_cast<unsigned long long*>(out_sizes + 2), 1ull);
    const int tiles = (opp_n + DL_NT - 1) / DL_NT;
    const int per = (tiles + slices - 1) / slices;
    const int t0 = blockIdx.y * per, t1 = min(t0 + per, tiles);
    if (t0 >= t1) return;                                              // the same for the whole workgroup
    unsigned gt = 0, eq = 0;
    for (int tile = t0; tile < t1; ++tile) {
        const int j = tile * DL_NT + (int)threadIdx.x;
        ts[threadIdx.x] = j < opp_n ? sign * s[order[opp_at + j]] : __uint_as_float(0x7FC00000u);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < DL_NT / 4; ++k) {                          // every lane reads the same 16 bytes: an LDS broadcast
            const float4 y = reinterpret_cast<const float4*>(ts)[k];
            gt += (unsigned)(x > y.x) + (unsigned)(x > y.y) + (unsigned)(x > y.z) + (unsigned)(x > y.w);
            eq += (unsigned)(x == y.x) + (unsigned)(x == y.y) + (unsigned)(x == y.z) + (unsigned)(x == y.w);
        }
        __syncthreads();
    }
    // b * 256 + thread < rows_cap = 256 * gridDim.x
    if (inside) atomicAdd(&cnt[(size_t)blockIdx.z * rows_cap + (size_t)b * DL_NT + threadIdx.x], 2u * gt + eq);
}

__global__ __launch_bounds__(DL_NT) void delong_reduce_kernel(const unsigned* __restrict__ cnt, int K, int rows_cap,
                                                              int64_t* __restrict__ out, const int64_t* __restrict__ out_sizes) {
    __shared__ long long buf[DL_NT];
    int k = 0, l = (int)blockIdx.x;                                    // pair index -> (k, l), k <= l, row-major upper triangle
    while (l >= K - k) {
        l -= K - k;
        ++k;
    }
    l += k;
    const int side = blockIdx.y;                                       // 0: the positives' rows (T, A), 1: the negatives' (T, B)
    const int m = (int)out_sizes[0], n0 = (int)out_sizes[1];
    const int rows = side ? n0 : m;
    const size_t first = side ? (size_t)((m + DL_NT - 1) / DL_NT) * DL_NT : 0;
    const unsigned* __restrict__ ck = cnt + (size_t)k * rows_cap + first;
    const unsigned* __restrict__ cl = cnt + (size_t)l * rows_cap + first;
    long long prod = 0, sum = 0;
    for (int r = threadIdx.x; r < rows; r += DL_NT) {
        const long long vk = ck[r], vl = cl[r];
        prod += vk * vl;
        sum += vk;
    }
    prod = block_tree_sum<DL_NT>(prod, buf);
    sum = block_tree_sum<DL_NT>(sum, buf);
    if (threadIdx.x != 0) return;
    const int P = K * (K + 1) / 2;
    out[2 * K + side * P + blockIdx.x] = prod;
    if (k == l) out[side * K + k] = sum;
}

bool in_range(int n, int K) { return n >= 2 && n <= DL_N_MAX && K >= 1 && K <= DL_K_MAX; }

}  // namespace

extern "C" size_t eoe_delong_scratch_bytes(int n, int K) {
    return in_range(n, K) ? order_bytes(n) + (size_t)K * row_blocks(n) * DL_NT * sizeof(unsigned) : 0;
}

extern "C" int eoe_delong_slices(int n, int K) { return in_range(n, K) ? slices_for(n, K) : 0; }

extern "C" int eoe_delong_counts(const float* scores, const int64_t* labels, int n, int K, int64_t* out, void* scratch, void* stream) {
    EOE_CHECK_ARG(scores, "delong_counts: null scores");
    EOE_CHECK_ARG(labels, "delong_counts: null labels");
    EOE_CHECK_ARG(out, "delong_counts: null out");
    EOE_CHECK_ARG(scratch, "delong_counts: null scratch");
    EOE_CHECK_ARG(n >= 2 && n <= DL_N_MAX, "delong_counts: n must be in [2, %d], not %d", DL_N_MAX, n);
    EOE_CHECK_ARG(K >= 1 && K <= DL_K_MAX, "delong_counts: K must be in [1, %d], not %d", DL_K_MAX, K);
    EOE_CHECK_ARG(((uintptr_t)scores & 3) == 0, "delong_counts: scores must be 4-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)labels & 7) == 0, "delong_counts: labels must be 8-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)out & 7) == 0, "delong_counts: out must be 8-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)scratch & 3) == 0, "delong_counts: scratch must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int P = pairs(K), blocks = row_blocks(n), rows_cap = blocks * DL_NT, slices = slices_for(n, K);
    char* base = static_cast<char*>(scratch);
    int* order = reinterpret_cast<int*>(base);
    unsigned* cnt = reinterpret_cast<unsigned*>(base + order_bytes(n));
    int64_t* out_sizes = out + 2 * K + 2 * P;
    ProfScope ps("delong_counts", 4.0 * (double)K * (double)n * (double)n / 2.0, 8.0 * (double)n + 12.0 * (double)K * (double)n, stream);
    // the row counters are added to; every slot of the table has one writer (the partition pass: the sizes, the reduce pass: the sums)
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)K * rows_cap * sizeof(unsigned), st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "delong_counts: clearing the counters: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(delong_partition_kernel, dim3(1), dim3(DL_PART_NT), 0, st, labels, n, order, out_sizes);
    EOE_CHECK_LAUNCH("delong_counts (partition)");
    hipLaunchKernelGGL(delong_count_kernel, dim3(blocks, slices, K), dim3(DL_NT), 0, st, scores, (const int*)order, n, slices, rows_cap, cnt,
                       out_sizes);
    EOE_CHECK_LAUNCH("delong_counts (count)");
    hipLaunchKernelGGL(delong_reduce_kernel, dim3(P, 2), dim3(DL_NT), 0, st, (const unsigned*)cnt, K, rows_cap, out,
                       (const int64_t*)out_sizes);
    EOE_CHECK_LAUNCH("delong_counts (reduce)");
    return 0;
}
