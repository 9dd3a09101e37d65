// The stratified, paired bootstrap of AUC, AP and FPR at a TPR level over K score columns of the same n samples: per replicate and
// column three numbers, counted on the device from draws that are stated exactly (include/eoe_hip.h), so that a NumPy restatement
// gives the same integers.  Positives are the samples with label 1 (m of them), negatives those with label 0 (n0); every other label
// is in neither.  The used samples are numbered u = 0 .. N-1 (N = m + n0): the positives in ascending sample index, then the negatives.
//
//   partition pass   ONE workgroup of 1 024 threads, as in delong.hip: `order[u]` = the sample index of used sample u; m, n0, a cleared
//                    NaN counter and the place of the TPR level go to the device, where the later passes read them.
//   rank pass        per column the position of every used sample in ascending score order, without a sort: position = #{v: s_v < s_u}
//                    + #{v < u: s_v == s_u}.  Rows in blocks of 256, one row per lane; a workgroup is (row block, slice of the tiles,
//                    column) and walks its slice in 256-score LDS tiles read back as 16-byte broadcasts.  A tile below the row block
//                    counts `<=`, one above it `<`, and only the diagonal tile compares indices.  A slice adds (less << 32) + equal-
//                    below to the row's 64-bit counter with one integer atomic.  Slice 0 counts the NaN scores.
//   place pass       position p = less + equal-below of sample u: posof[k][u] = p, and flags[k][p] = (is positive) | (first of its group
//                    of equal scores) << 1 -- a sample starts its group exactly when no equal score lies below it in the tie order.
//   replicate pass   workgroup (replicate b, column k) of 1 024 threads; b = B is the full sample, every multiplicity 1.  Per chunk of BS_CHUNK positions: clear the chunk's counters
//                    in LDS, regenerate ALL draws of the replicate from the Philox counter and count those that land in the chunk with
//                    integer LDS atomics (the multiplicity c[p] per sorted position), then scan.  Thread t owns 16 consecutive
//                    positions; the state in front of a position is (P, N, gP, gN): the weighted positives and negatives below it, and
//                    the same at the start of its group of equal scores.  A segment maps the state by (P + sp, N + sn, has ? P + lp :
//                    gP, has ? N + ln : gN) -- `has`: it holds a group start, lp / ln: its weights in front of the last one -- and these
//                    maps compose associatively: a wave scan by shuffles, the 16 wave totals through LDS, the chunk's carry in front.
//                    Then every thread replays its segment:
//                        positive p:  U2 += c gN;  ap += c / m * ((m - gP) / ((m - gP) + (n0 - gN)));  the positive whose weighted
//                                     places [P, P + c) hold m - place sets fps = n0 - gN
//                        negative p:  U2 += c (m - gP)
//                    (sum over pairs of [s_i > s_j] + [s_i >= s_j]; m - gP and n0 - gN are the cumulative counts of the descending
//                    curve at the group).  U2 in int64 and ap in float64, each thread in position order, then a fixed tree over the
//                    threads and the chunks in order: the same bytes on every run.  No floating-point atomics.
// One memset and four launches on the caller's stream; nothing in the scratch grows with B.
//
// Ranges: a counter half is at most N <= 2^20; the weighted sums are at most max(m, n0) <= 2^20 (int32); U2 <= 2 m n0 < 2^41.
// With a NaN among the used scores two samples may share a position: every index stays in range, the tables are unspecified.
#include "common.h"

namespace {

constexpr int BS_NT = 256;                     // rank pass: threads per workgroup = rows per block = scores per LDS tile
constexpr int BS_PART_NT = 1024;               // partition pass: one workgroup
constexpr int BS_REP_NT = 1024;                // replicate pass
constexpr int BS_SEG = 16;                     // positions per thread and chunk
constexpr int BS_CHUNK = BS_REP_NT * BS_SEG;   // sorted positions per LDS chunk: 16 384 (17 408 words with the padding: 2 workgroups per CU)
constexpr int BS_N_MAX = 1 << 20;
constexpr int BS_K_MAX = 8;
constexpr int BS_B_MAX = 65536;
constexpr int BS_TARGET_WGS = 2048;            // rank pass: slices are added until the grid has about this many workgroups ...
constexpr int BS_MAX_SLICES = 64;              // ... but never more than this

static_assert(BS_CHUNK == EOE_BOOTSTRAP_CHUNK, "the header states the chunk");

size_t order_bytes(int n) { return align_up((size_t)n * 4, 256); }
size_t flag_stride(int n) { return align_up((size_t)n, 256); }
int row_blocks(int n) { return cdiv(n, BS_NT); }
int slices_for(int n, int K) {
    const int s = cdiv(BS_TARGET_WGS, row_blocks(n) * K);
    return s < 1 ? 1 : (s > BS_MAX_SLICES ? BS_MAX_SLICES : s);
}
// scratch: order int32 [n] | cnt uint64 [K][rows_cap] | posof int32 [K][rows_cap] | flags uint8 [K][flag_stride] | place int32
size_t cnt_bytes(int n, int K) { return (size_t)K * row_blocks(n) * BS_NT * 8; }
size_t posof_bytes(int n, int K) { return (size_t)K * row_blocks(n) * BS_NT * 4; }
size_t flags_bytes(int n, int K) { return (size_t)K * flag_stride(n); }

// Philox4x32-10 (Salmon et al. 2011)
__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the smallest integer p with p / m >= tpr in float64 (metrics.place_for_tpr); 0 without positives
__device__ int place_for_tpr(double tpr, int m) {
    if (m < 1) return 0;
    double c = ceil(tpr * (double)m);
    int p = c < 1.0 ? 1 : (c > (double)m ? m : (int)c);
    while (p > 1 && (double)(p - 1) / (double)m >= tpr) --p;
    while (p < m && (double)p / (double)m < tpr) ++p;
    return p;
}

__global__ __launch_bounds__(BS_PART_NT) void bootstrap_partition_kernel(const int64_t* __restrict__ labels, int n, double tpr,
                                                                         int* __restrict__ order, int* __restrict__ counts,
                                                                         int* __restrict__ place) {
    __shared__ int sp[2][BS_PART_NT];
    __shared__ int sq[2][BS_PART_NT];
    const int t = threadIdx.x;
    const int chunk = (n + BS_PART_NT - 1) / BS_PART_NT;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int p = 0, q = 0;
    for (int i = lo; i < hi; ++i) {
        const int64_t y = labels[i];
        p += y == 1;
        q += y == 0;
    }
    int cur = 0;
    sp[0][t] = p;
    sq[0][t] = q;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < BS_PART_NT; d <<= 1) {
        const int vp = sp[cur][t] + (t >= d ? sp[cur][t - d] : 0);
        const int vq = sq[cur][t] + (t >= d ? sq[cur][t - d] : 0);
        sp[cur ^ 1][t] = vp;
        sq[cur ^ 1][t] = vq;
        cur ^= 1;
        __syncthreads();
    }
    const int m = sp[cur][BS_PART_NT - 1], n0 = sq[cur][BS_PART_NT - 1];
    int at_p = sp[cur][t] - p, at_q = m + sq[cur][t] - q;              // < m and < m + n0 <= n while there is something to write
    for (int i = lo; i < hi; ++i) {
        const int64_t y = labels[i];
        if (y == 1) order[at_p++] = i;
        else if (y == 0) order[at_q++] = i;
    }
    if (t == 0) {
        counts[0] = m;
        counts[1] = n0;
        counts[2] = 0;                                                 // the NaN counter of the rank pass
        if (place) *place = place_for_tpr(tpr, m);
    }
}

__global__ __launch_bounds__(BS_NT) void bootstrap_rank_kernel(const float* __restrict__ scores, const int* __restrict__ order, int n,
                                                               int slices, int rows_cap, unsigned long long* __restrict__ cnt,
                                                               int* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float ts[BS_NT];
    const int N = counts[0] + counts[1];                               // written by the partition pass: N <= n
    const int b = blockIdx.x;
    if (b * BS_NT >= N) return;                                        // the grid is sized for N = n
    const float nan = __uint_as_float(0x7FC00000u);
    const float* __restrict__ s = scores + (size_t)blockIdx.z * n;
    const int u = b * BS_NT + (int)threadIdx.x;
    const bool inside = u < N;
    const float x = inside ? s[order[u]] : nan;
    if (blockIdx.y == 0 && inside && x != x) atomicAdd(counts + 2, 1);
    const int tiles = (N + BS_NT - 1) / BS_NT;
    const int per = (tiles + slices - 1) / slices;
    const int t0 = blockIdx.y * per, t1 = min(t0 + per, tiles);
    if (t0 >= t1) return;                                              // the same for the whole workgroup
    unsigned lt = 0, eq = 0;
    for (int tile = t0; tile < t1; ++tile) {
        const int v = tile * BS_NT + (int)threadIdx.x;
        ts[threadIdx.x] = v < N ? s[order[v]] : nan;                   // the padding compares false
        __syncthreads();
        if (tile != b) {
            // every v of a tile below the row block is below every u of it: an equal score there counts; above, it does not
            const bool below = tile < b;
#pragma unroll 8
            for (int k = 0; k < BS_NT / 4; ++k) {                      // every lane reads the same 16 bytes: an LDS broadcast
                const float4 y = reinterpret_cast<const float4*>(ts)[k];
                lt += (unsigned)(y.x < x) + (unsigned)(y.y < x) + (unsigned)(y.z < x) + (unsigned)(y.w < x);
                if (below) eq += (unsigned)(y.x == x) + (unsigned)(y.y == x) + (unsigned)(y.z == x) + (unsigned)(y.w == x);
            }
        } else {
            const int me = (int)threadIdx.x;
#pragma unroll 8
            for (int k = 0; k < BS_NT / 4; ++k) {
                const float4 y = reinterpret_cast<const float4*>(ts)[k];
                lt += (unsigned)(y.x < x) + (unsigned)(y.y < x) + (unsigned)(y.z < x) + (unsigned)(y.w < x);
                eq += (unsigned)(y.x == x && 4 * k < me) + (unsigned)(y.y == x && 4 * k + 1 < me) + (unsigned)(y.z == x && 4 * k + 2 < me) +
                      (unsigned)(y.w == x && 4 * k + 3 < me);
            }
        }
        __syncthreads();
    }
    // u < rows_cap = 256 * gridDim.x
    if (inside) atomicAdd(&cnt[(size_t)blockIdx.z * rows_cap + u], ((unsigned long long)lt << 32) | (unsigned long long)eq);
}

__global__ __launch_bounds__(BS_NT) void bootstrap_place_kernel(const unsigned long long* __restrict__ cnt, int rows_cap, size_t fstride,
                                                                int* __restrict__ posof, uint8_t* __restrict__ flags,
                                                                const int* __restrict__ counts) {
    const int m = counts[0], N = m + counts[1];
    const int u = blockIdx.x * BS_NT + (int)threadIdx.x;
    if (u >= N) return;
    const size_t k = blockIdx.y;
    const unsigned long long c = cnt[k * rows_cap + u];
    const unsigned lt = (unsigned)(c >> 32), eq = (unsigned)c;
    unsigned p = lt + eq;                                              // < N: the sample itself is in neither count
    if (p >= (unsigned)N) p = (unsigned)N - 1;                         // never taken; keeps a broken count inside the row
    posof[k * rows_cap + u] = (int)p;
    flags[k * fstride + p] = (uint8_t)((u < m ? 1 : 0) | (eq == 0 ? 2 : 0));
}

// how a run of positions maps the state in front of it: see the head of the file
struct Seg {
    int sp, sn, lp, ln, has;
};
__device__ __forceinline__ Seg compose(const Seg& a, const Seg& b) {   // a, then b
    Seg r;
    r.sp = a.sp + b.sp;
    r.sn = a.sn + b.sn;
    r.lp = b.has ? a.sp + b.lp : a.lp;
    r.ln = b.has ? a.sn + b.ln : a.ln;
    r.has = a.has | b.has;
    return r;
}
__device__ __forceinline__ Seg shfl_up_seg(const Seg& a, int d) {
    Seg r;
    r.sp = __shfl_up(a.sp, d, 64);
    r.sn = __shfl_up(a.sn, d, 64);
    r.lp = __shfl_up(a.lp, d, 64);
    r.ln = __shfl_up(a.ln, d, 64);
    r.has = __shfl_up(a.has, d, 64);
    return r;
}

// a position's counter: 16 consecutive positions of a thread sit 17 words from the next thread's, so that the replay's reads
// (lane l at word 17 l + i) fall on 32 different banks
__device__ __forceinline__ int padded(int p) { return p + (p >> 4); }

__global__ __launch_bounds__(BS_REP_NT, 8) void bootstrap_replicate_kernel(const int* __restrict__ posof, const uint8_t* __restrict__ flags,
                                                                        int rows_cap, size_t fstride, int B, unsigned key0, unsigned key1,
                                                                        const int* __restrict__ counts, const int* __restrict__ place,
                                                                        int64_t* __restrict__ out_u2, int64_t* __restrict__ out_fps,
                                                                        double* __restrict__ out_ap) {
    __shared__ __attribute__((aligned(16))) unsigned cnt[BS_CHUNK + BS_CHUNK / BS_SEG];
    __shared__ Seg wave_tot[BS_REP_NT / 64];
    __shared__ Seg carry;
    __shared__ int s_fps;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x;
    const size_t k = blockIdx.y;
    const int m = counts[0], n0 = counts[1], N = m + n0;
    const size_t o = k * (size_t)(B + 1) + b;
    if (m == 0 || n0 == 0) {                                           // the same for the whole workgroup
        if (t == 0) {
            out_u2[o] = 0;
            out_fps[o] = 0;
            out_ap[o] = 0.0;
        }
        return;
    }
    const int target = m - *place;                                     // the ascending weighted place of the threshold's positive, in [0, m)
    const int* __restrict__ pk = posof + k * rows_cap;
    const uint8_t* __restrict__ fk = flags + k * fstride;
    const int calls_p = (m + 3) >> 2, calls = calls_p + ((n0 + 3) >> 2);
    if (t == 0) {
        carry = Seg{0, 0, 0, 0, 1};
        s_fps = 0;
    }
    long long u2 = 0;
    double ap = 0.0;
    const double dm = (double)m;
    for (int c0 = 0; c0 < N; c0 += BS_CHUNK) {
        for (int i = t; i < BS_CHUNK + BS_CHUNK / BS_SEG; i += BS_REP_NT) cnt[i] = 0u;
        __syncthreads();
        if (b == B) {                                                  // the full sample: every multiplicity is 1
            for (int i = t; i < BS_CHUNK; i += BS_REP_NT)
                if (c0 + i < N) cnt[padded(i)] = 1u;
        }
        for (int call = t; call < (b == B ? 0 : calls); call += BS_REP_NT) {
            const bool pos = call < calls_p;
            const int j = pos ? call : call - calls_p, size = pos ? m : n0, at = pos ? 0 : m;
            unsigned w[4];
            philox4x32((unsigned)j, (unsigned)b, pos ? 1u : 0u, 0u, key0, key1, w);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (4 * j + q < size) {                                // the unused words of the last call are dropped
                    const int at_u = at + (int)(((unsigned long long)w[q] * (unsigned long long)size) >> 32);      // < at + size <= N
                    const unsigned p = (unsigned)(pk[at_u] - c0);      // posof < N
                    if (p < (unsigned)BS_CHUNK) atomicAdd(&cnt[padded((int)p)], 1u);
                }
            }
        }
        __syncthreads();
        // the thread's segment: positions c0 + 16 t .. + 15, those below N
        const int p0 = c0 + t * BS_SEG;
        const int len = min(BS_SEG, N - p0);                           // <= 0: nothing
        unsigned c[BS_SEG];
        uint8_t f[BS_SEG];
        Seg mine = Seg{0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < BS_SEG; ++i) {
            const bool in = i < len;
            c[i] = in ? cnt[t * (BS_SEG + 1) + i] : 0u;
            f[i] = in ? fk[p0 + i] : (uint8_t)0;
            if (f[i] & 2) {
                mine.has = 1;
                mine.lp = mine.sp;
                mine.ln = mine.sn;
            }
            if (f[i] & 1) mine.sp += (int)c[i];
            else mine.sn += (int)c[i];
        }
        // inclusive scan over the wave, then the waves in front and the chunk's carry
        Seg inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Seg other = shfl_up_seg(inc, d);
            if (lane >= d) inc = compose(other, inc);
        }
        if (lane == 63) wave_tot[wave] = inc;
        Seg exc = shfl_up_seg(inc, 1);
        if (lane == 0) exc = Seg{0, 0, 0, 0, 0};
        __syncthreads();
        Seg front = carry;
        for (int w = 0; w < wave; ++w) front = compose(front, wave_tot[w]);
        const Seg st = compose(front, exc);
        int P = st.sp, Nn = st.sn, gP = st.lp, gN = st.ln;
#pragma unroll
        for (int i = 0; i < BS_SEG; ++i) {
            if (f[i] & 2) {
                gP = P;
                gN = Nn;
            }
            const int ci = (int)c[i];
            if (ci != 0) {
                if (f[i] & 1) {
                    u2 += (long long)ci * gN;
                    const double tps = (double)(m - gP), fps = (double)(n0 - gN);
                    ap += (double)ci / dm * (tps / (tps + fps));
                    if (P <= target && target < P + ci) s_fps = n0 - gN;          // one positive in the whole replicate
                    P += ci;
                } else {
                    u2 += (long long)ci * (long long)(m - gP);
                    Nn += ci;
                }
            }
        }
        __syncthreads();                                               // every thread has read the carry and the wave totals
        if (t == BS_REP_NT - 1) carry = Seg{P, Nn, gP, gN, 1};
        // the next chunk's clearing pass is followed by a barrier before anything reads `carry` or writes `cnt` entries again
    }
    // the counters were last read in front of the loop's last barrier: their words carry the two sums over the threads
    static_assert(sizeof(cnt) >= BS_REP_NT * 8, "the tree sums reuse the counters");
    const long long u2_all = block_tree_sum<BS_REP_NT>(u2, reinterpret_cast<long long*>(cnt));
    const double ap_all = block_tree_sum<BS_REP_NT>(ap, reinterpret_cast<double*>(cnt));
    if (t == 0) {
        out_u2[o] = u2_all;
        out_fps[o] = s_fps;
        out_ap[o] = ap_all;
    }
}

__global__ __launch_bounds__(BS_NT) void bootstrap_draws_kernel(const int* __restrict__ order, int b, unsigned key0, unsigned key1,
                                                                const int* __restrict__ counts, int* __restrict__ out) {
    const int m = counts[0], n0 = counts[1];
    const int calls_p = (m + 3) >> 2, calls = calls_p + ((n0 + 3) >> 2);
    for (int call = blockIdx.x * BS_NT + (int)threadIdx.x; call < calls; call += gridDim.x * BS_NT) {
        const bool pos = call < calls_p;
        const int j = pos ? call : call - calls_p, size = pos ? m : n0, at = pos ? 0 : m;
        unsigned w[4];
        philox4x32((unsigned)j, (unsigned)b, pos ? 1u : 0u, 0u, key0, key1, w);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * j + q < size)                                      // order[< m + n0] < n
                atomicAdd(&out[order[at + (int)(((unsigned long long)w[q] * (unsigned long long)size) >> 32)]], 1);
    }
}

bool in_range(int n, int K, int B) { return n >= 2 && n <= BS_N_MAX && K >= 1 && K <= BS_K_MAX && B >= 1 && B <= BS_B_MAX; }

}  // namespace

extern "C" size_t eoe_bootstrap_scratch_bytes(int n, int K, int B) {
    return in_range(n, K, B) ? order_bytes(n) + cnt_bytes(n, K) + posof_bytes(n, K) + flags_bytes(n, K) + 256 : 0;
}

extern "C" int eoe_bootstrap_counts(const float* scores, const int64_t* labels, int n, int K, int B, uint64_t seed, double tpr,
                                    int64_t* out_u2, int64_t* out_fps, double* out_ap, int32_t* counts, void* scratch, void* stream) {
    EOE_CHECK_ARG(scores, "bootstrap_counts: null scores");
    EOE_CHECK_ARG(labels, "bootstrap_counts: null labels");
    EOE_CHECK_ARG(out_u2 && out_fps && out_ap, "bootstrap_counts: null output table");
    EOE_CHECK_ARG(counts, "bootstrap_counts: null counts");
    EOE_CHECK_ARG(scratch, "bootstrap_counts: null scratch");
    EOE_CHECK_ARG(n >= 2 && n <= BS_N_MAX, "bootstrap_counts: n must be in [2, %d], not %d", BS_N_MAX, n);
    EOE_CHECK_ARG(K >= 1 && K <= BS_K_MAX, "bootstrap_counts: K must be in [1, %d], not %d", BS_K_MAX, K);
    EOE_CHECK_ARG(B >= 1 && B <= BS_B_MAX, "bootstrap_counts: B must be in [1, %d], not %d", BS_B_MAX, B);
    EOE_CHECK_ARG(tpr > 0.0 && tpr <= 1.0, "bootstrap_counts: tpr must be in (0, 1], not %g", tpr);
    EOE_CHECK_ARG(((uintptr_t)scores & 3) == 0 && ((uintptr_t)counts & 3) == 0, "bootstrap_counts: scores and counts must be 4-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)labels & 7) == 0 && ((uintptr_t)out_u2 & 7) == 0 && ((uintptr_t)out_fps & 7) == 0 && ((uintptr_t)out_ap & 7) == 0,
                  "bootstrap_counts: labels and the output tables must be 8-byte aligned");
    EOE_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "bootstrap_counts: scratch must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = row_blocks(n), rows_cap = blocks * BS_NT, slices = slices_for(n, K);
    const size_t fstride = flag_stride(n);
    char* base = static_cast<char*>(scratch);
    int* order = reinterpret_cast<int*>(base);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base + order_bytes(n));
    int* posof = reinterpret_cast<int*>(base + order_bytes(n) + cnt_bytes(n, K));
    uint8_t* flags = reinterpret_cast<uint8_t*>(base + order_bytes(n) + cnt_bytes(n, K) + posof_bytes(n, K));
    int* place = reinterpret_cast<int*>(base + order_bytes(n) + cnt_bytes(n, K) + posof_bytes(n, K) + flags_bytes(n, K));
    ProfScope ps("bootstrap_counts", 3.0 * (double)K * (double)n * (double)n + 20.0 * (double)B * (double)K * (double)n,
                 8.0 * (double)n + 4.0 * (double)K * (double)n + 5.0 * (double)B * (double)K * (double)n, stream);
    hipError_t e = hipMemsetAsync(cnt, 0, cnt_bytes(n, K), st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "bootstrap_counts: clearing the counters: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(bootstrap_partition_kernel, dim3(1), dim3(BS_PART_NT), 0, st, labels, n, tpr, order, (int*)counts, place);
    EOE_CHECK_LAUNCH("bootstrap_counts (partition)");
    hipLaunchKernelGGL(bootstrap_rank_kernel, dim3(blocks, slices, K), dim3(BS_NT), 0, st, scores, (const int*)order, n, slices, rows_cap, cnt,
                       (int*)counts);
    EOE_CHECK_LAUNCH("bootstrap_counts (rank)");
    hipLaunchKernelGGL(bootstrap_place_kernel, dim3(blocks, K), dim3(BS_NT), 0, st, (const unsigned long long*)cnt, rows_cap, fstride, posof,
                       flags, (const int*)counts);
    EOE_CHECK_LAUNCH("bootstrap_counts (place)");
    hipLaunchKernelGGL(bootstrap_replicate_kernel, dim3(B + 1, K), dim3(BS_REP_NT), 0, st, (const int*)posof, (const uint8_t*)flags, rows_cap,
                       fstride, B, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (const int*)counts, (const int*)place, out_u2,
                       out_fps, out_ap);
    EOE_CHECK_LAUNCH("bootstrap_counts (replicate)");
    return 0;
}

extern "C" int eoe_bootstrap_draws(const int64_t* labels, int n, int b, uint64_t seed, int32_t* out, void* scratch, void* stream) {
    EOE_CHECK_ARG(labels, "bootstrap_draws: null labels");
    EOE_CHECK_ARG(out, "bootstrap_draws: null out");
    EOE_CHECK_ARG(scratch, "bootstrap_draws: null scratch");
    EOE_CHECK_ARG(n >= 2 && n <= BS_N_MAX, "bootstrap_draws: n must be in [2, %d], not %d", BS_N_MAX, n);
    EOE_CHECK_ARG(b >= 0 && b < BS_B_MAX, "bootstrap_draws: b must be in [0, %d), not %d", BS_B_MAX, b);
    EOE_CHECK_ARG(((uintptr_t)labels & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)scratch & 7) == 0,
                  "bootstrap_draws: labels and scratch must be 8-byte aligned, out 4-byte");
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(scratch);
    int* order = reinterpret_cast<int*>(base);
    int* counts = reinterpret_cast<int*>(base + order_bytes(n));       // the head of the counters' region: 3 words
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 4, st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "bootstrap_draws: clearing the output: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(bootstrap_partition_kernel, dim3(1), dim3(BS_PART_NT), 0, st, labels, n, 1.0, order, counts, (int*)nullptr);
    EOE_CHECK_LAUNCH("bootstrap_draws (partition)");
    const int grid = min(cdiv(cdiv(n, 4) + 1, BS_NT), 1024);
    hipLaunchKernelGGL(bootstrap_draws_kernel, dim3(grid), dim3(BS_NT), 0, st, (const int*)order, b, (unsigned)(seed & 0xffffffffull),
                       (unsigned)(seed >> 32), (const int*)counts, out);
    EOE_CHECK_LAUNCH("bootstrap_draws");
    return 0;
}
