// The extremes of the test scores on the device: per label group the k highest and the k lowest scores with their positions (the
// reference ranks OE individuals this way in `Tree.scores_best` / `imsave_best`, and leaves the test scores to a per-sample JSON the
// user sorts by hand).  Four lists: (group 0, group 1) x (most, least); list l = 2 * group + end.
//
//   key           every member of a group gets one 52-bit integer per end: the order-preserving 32-bit image of its score (ordered_bits: -0.0 folded
//                 into 0.0; the image complemented for the "most" end) above its 20-bit position.  Keys of one list are distinct, and
//                 ascending key order is the list's order -- descending (most) or ascending (least) by score, equal scores by
//                 ascending position: what np.argsort(-s, kind="stable") and np.argsort(s, kind="stable") give.  A list is the
//                 k' = min(k, group size) smallest keys, sorted.
//   select        five digit passes over the n scores, 11 + 11 + 10 + 10 + 10 bits from the top: a pass counts, per list, the digit of
//                 the keys that carry the prefix found so far (LDS integer atomics, the non-zero counters folded into the pass's own
//                 global table by integer adds).  The next launch starts by narrowing: wave l scans list l's table for the digit
//                 that holds the rank it looks for, every workgroup for itself (integers: all of them find the same), and workgroup 0
//                 leaves the new (prefix, rank) in scratch for the launch after it.  Nothing comes back to the host in between.
//   gather        a sixth pass narrows the last digit -- the prefix is now the k'-th smallest key itself -- and appends every key
//                 <= it to the list's buffer through a slot counter: exactly k' keys, in any order.
//   sort          one workgroup per list sorts its at most 1 024 keys in LDS (bitonic) and writes position and the score's own bits.
// Integer compares and integer adds only: two runs give the same bytes.  n log-free: 6 reads of the scores, no n^2 pass.
// Eight enqueues on the caller's stream: one memset (the count tables and slot counters) and seven launches.
#include "common.h"

namespace {

constexpr int TK_NT = 256;                     // select / gather: 4 waves, wave l narrows list l
constexpr int TK_LISTS = 4;
constexpr int TK_BINS = 2048;                  // counters per list and pass (the 10-bit passes use the first 1 024)
constexpr int TK_PASSES = 5;
constexpr int TK_K_MAX = 1024;                 // what one workgroup sorts in LDS
constexpr int TK_N_MAX = 1 << 20;              // positions fit the key's low 20 bits
constexpr int TK_IDX_BITS = 20;
constexpr int TK_MAX_GRID = 256;

__host__ __device__ constexpr int pass_bits(int p) { return p < 2 ? 11 : 10; }
__host__ __device__ constexpr int pass_shift(int p) { return p == 0 ? 41 : (p == 1 ? 30 : (p == 2 ? 20 : (p == 3 ? 10 : 0))); }

struct TkState {                               // a list after a narrowing: the key's leading digits and the rank among the keys that carry them
    unsigned long long prefix;
    unsigned rank;                             // 1-based; 0 = nothing to select (empty group)
    unsigned pad;
};

// scratch layout (bytes); [0, TK_ZERO_BYTES) is cleared by the memset
constexpr size_t TK_OFF_HIST = 0;                                                           // unsigned [5][4][2048]
constexpr size_t TK_OFF_CNT = TK_OFF_HIST + (size_t)TK_PASSES * TK_LISTS * TK_BINS * 4;     // unsigned [4] slot counters, [1] non-finite, [3] unused
constexpr size_t TK_ZERO_BYTES = TK_OFF_CNT + 8 * 4;
constexpr size_t TK_OFF_STATE = TK_ZERO_BYTES;                                              // TkState [5][4]
constexpr size_t TK_OFF_META = TK_OFF_STATE + (size_t)TK_PASSES * TK_LISTS * sizeof(TkState);   // unsigned [2] group sizes, [2] unused
constexpr size_t TK_OFF_KEYS = TK_OFF_META + 4 * 4;                                         // unsigned long long [4][1024]
constexpr size_t TK_SCRATCH_BYTES = TK_OFF_KEYS + (size_t)TK_LISTS * TK_K_MAX * 8;

int topk_grid(int n) { const int g = cdiv(n, TK_NT * 4); return g < TK_MAX_GRID ? g : TK_MAX_GRID; }

__device__ __forceinline__ unsigned long long make_key(unsigned u, int end, unsigned i) {
    return ((unsigned long long)(end == 0 ? ~u : u) << TK_IDX_BITS) | i;
}
__device__ __forceinline__ int group_of(const int64_t* __restrict__ labels, int i) {
    if (!labels) return 0;
    const int64_t y = labels[i];
    return y == 0 ? 0 : (y == 1 ? 1 : -1);       // any other label, e.g. -1 for unlabelled images, is in neither group
}

// Wave l narrows list l by the table `hist` of the pass over `bits` bits: the digit d with (count below d) < rank <= (count up to d)
// extends the prefix, and the rank becomes its place inside that digit.  `first`: the table is the first pass's, the rank starts as
// min(k, group size) and workgroup 0 records the group size.  Lane j holds 32 consecutive counters; an inclusive scan over the lanes.
__device__ __forceinline__ void narrow(const unsigned* __restrict__ hist, int bits, bool first, int k, const TkState* __restrict__ prev,
                                       TkState* __restrict__ s_out, unsigned* __restrict__ meta) {
    const int lane = threadIdx.x & 63, l = threadIdx.x >> 6;
    const uint4* h4 = reinterpret_cast<const uint4*>(hist + (size_t)l * TK_BINS + lane * 32);
    unsigned v[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 t = h4[q];
        v[4 * q + 0] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    unsigned local = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) local += v[j];
    unsigned incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const unsigned total = __shfl(incl, 63, 64);
    unsigned long long prefix = 0ull;
    unsigned rank;
    if (first) {
        rank = total < (unsigned)k ? total : (unsigned)k;
        if (blockIdx.x == 0 && lane == 0 && (l & 1) == 0) meta[l >> 1] = total;
    } else {
        prefix = prev[l].prefix;
        rank = prev[l].rank;
    }
    const unsigned excl = incl - local;
    const bool hit = rank >= 1u && excl < rank && rank <= incl;
    if (__ballot(hit) == 0ull) {                 // an empty group, or a rank no table holds: nothing is selected from this list
        if (lane == 0) s_out[l] = TkState{prefix << bits, 0u, 0u};
    } else if (hit) {                            // one lane: the counters are a partition of the keys that carry the prefix
        unsigned cum = excl, d = 0, r = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if (!found && cum + v[j] >= rank) {
                found = true;
                d = (unsigned)(lane * 32 + j);
                r = rank - cum;
            }
            cum += v[j];
        }
        s_out[l] = TkState{(prefix << bits) | d, r, 0u};
    }
}

// pass P: narrows by pass P - 1's table (P > 0), then counts digit P of the keys that carry the prefix
__global__ __launch_bounds__(TK_NT) void topk_pass_kernel(const float* __restrict__ s, const int64_t* __restrict__ labels, int n, int k,
                                                          int P, unsigned* __restrict__ hist_all, TkState* __restrict__ state_all,
                                                          unsigned* __restrict__ meta, unsigned* __restrict__ nonfinite) {
    __shared__ unsigned sc[TK_LISTS * TK_BINS];
    __shared__ TkState st[TK_LISTS];
    __shared__ unsigned s_nf;
    for (int i = threadIdx.x; i < TK_LISTS * TK_BINS; i += TK_NT) sc[i] = 0u;
    if (threadIdx.x == 0) s_nf = 0u;
    if (P > 0) {
        narrow(hist_all + (size_t)(P - 1) * TK_LISTS * TK_BINS, pass_bits(P - 1), P == 1, k, state_all + (P > 1 ? (P - 2) * TK_LISTS : 0), st,
               meta);
    }
    __syncthreads();
    if (P > 0 && blockIdx.x == 0 && threadIdx.x < TK_LISTS) state_all[(P - 1) * TK_LISTS + threadIdx.x] = st[threadIdx.x];
    const int shift = pass_shift(P), bits = pass_bits(P);
    const unsigned mask = (1u << bits) - 1u;
    const int stride = (int)gridDim.x * TK_NT;
    for (int i = (int)blockIdx.x * TK_NT + (int)threadIdx.x; i < n; i += stride) {
        const int g = group_of(labels, i);
        if (g < 0) continue;
        const float x = s[i];
        const unsigned u = ordered_bits(x);
        if (P == 0 && ::nonfinite(x)) atomicAdd(&s_nf, 1u);          // the function of common.h, not the counter
#pragma unroll
        for (int end = 0; end < 2; ++end) {
            const int l = 2 * g + end;
            const unsigned long long key = make_key(u, end, (unsigned)i);
            const unsigned d = (unsigned)(key >> shift) & mask;
            if (P == 0) {
                atomicAdd(&sc[l * TK_BINS + d], 1u);
            } else if (st[l].rank != 0u && (key >> (shift + bits)) == st[l].prefix) {
                atomicAdd(&sc[l * TK_BINS + d], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* hist = hist_all + (size_t)P * TK_LISTS * TK_BINS;
    for (int i = threadIdx.x; i < TK_LISTS * TK_BINS; i += TK_NT) {
        const unsigned c = sc[i];
        if (c) atomicAdd(&hist[i], c);
    }
    if (P == 0 && threadIdx.x == 0 && s_nf) atomicAdd(nonfinite, s_nf);
}

// narrows by the last pass's table -- the prefix is then the threshold key -- and collects the keys up to it
__global__ __launch_bounds__(TK_NT) void topk_gather_kernel(const float* __restrict__ s, const int64_t* __restrict__ labels, int n, int k,
                                                            const unsigned* __restrict__ hist_all, TkState* __restrict__ state_all,
                                                            unsigned* __restrict__ meta, unsigned* __restrict__ cnt,
                                                            unsigned long long* __restrict__ keys) {
    __shared__ TkState st[TK_LISTS];
    narrow(hist_all + (size_t)(TK_PASSES - 1) * TK_LISTS * TK_BINS, pass_bits(TK_PASSES - 1), false, k,
           state_all + (TK_PASSES - 2) * TK_LISTS, st, meta);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < TK_LISTS) state_all[(TK_PASSES - 1) * TK_LISTS + threadIdx.x] = st[threadIdx.x];
    unsigned want[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) want[g] = meta[g] < (unsigned)k ? meta[g] : (unsigned)k;
    const int stride = (int)gridDim.x * TK_NT;
    for (int i = (int)blockIdx.x * TK_NT + (int)threadIdx.x; i < n; i += stride) {
        const int g = group_of(labels, i);
        if (g < 0) continue;
        const unsigned u = ordered_bits(s[i]);
#pragma unroll
        for (int end = 0; end < 2; ++end) {
            const int l = 2 * g + end;
            const unsigned long long key = make_key(u, end, (unsigned)i);
            if (st[l].rank != 0u && key <= st[l].prefix) {
                const unsigned slot = atomicAdd(&cnt[l], 1u);
                if (slot < want[g] && slot < (unsigned)TK_K_MAX) keys[(size_t)l * TK_K_MAX + slot] = key;   // exactly want[g] keys qualify
            }
        }
    }
}

// workgroup l: list l's keys ascending (bitonic over the next power of two, the tail padded with the largest key), then position and score
__global__ __launch_bounds__(TK_K_MAX) void topk_sort_kernel(const float* __restrict__ s, int n, int k, const unsigned* __restrict__ meta,
                                                             const unsigned* __restrict__ cnt, const unsigned* __restrict__ nonfinite,
                                                             const unsigned long long* __restrict__ keys, int32_t* __restrict__ out_idx,
                                                             float* __restrict__ out_val, int32_t* __restrict__ out_counts) {
    __shared__ unsigned long long sk[TK_K_MAX];
    const int l = blockIdx.x, g = l >> 1, t = threadIdx.x;
    unsigned c = meta[g] < (unsigned)k ? meta[g] : (unsigned)k;
    c = cnt[l] < c ? cnt[l] : c;
    if (l == 0 && t < 3) out_counts[t] = t < 2 ? (int32_t)meta[t] : (int32_t)nonfinite[0];
    int pow2 = 2;
    while (pow2 < (int)c) pow2 <<= 1;
    sk[t] = (unsigned)t < c ? keys[(size_t)l * TK_K_MAX + t] : ~0ull;
    for (int size = 2; size <= pow2; size <<= 1) {
        for (int str = size >> 1; str > 0; str >>= 1) {
            __syncthreads();
            const int o = t ^ str;
            if (t < pow2 && o > t) {
                const unsigned long long a = sk[t], b = sk[o];
                if ((a > b) == ((t & size) == 0)) { sk[t] = b; sk[o] = a; }
            }
        }
    }
    __syncthreads();
    if ((unsigned)t < c) {
        const unsigned i = (unsigned)(sk[t] & ((1ull << TK_IDX_BITS) - 1ull));
        if (i < (unsigned)n) {
            out_idx[(size_t)l * k + t] = (int32_t)i;
            out_val[(size_t)l * k + t] = s[i];
        }
    }
}

bool in_range(int n, int k) { return n >= 1 && n <= TK_N_MAX && k >= 1 && k <= TK_K_MAX; }

}  // namespace

extern "C" size_t eoe_score_extremes_scratch_bytes(int n, int k) { return in_range(n, k) ? TK_SCRATCH_BYTES : 0; }

extern "C" int eoe_score_extremes(const float* scores, const int64_t* labels, int n, int k, int32_t* out_idx, float* out_val,
                                  int32_t* out_counts, void* scratch, void* stream) {
    EOE_CHECK_ARG(scores && out_idx && out_val && out_counts && scratch, "score_extremes: null scores, output or scratch");
    EOE_CHECK_ARG(n >= 1 && n <= TK_N_MAX, "score_extremes: n must be in [1, %d], not %d", TK_N_MAX, n);
    EOE_CHECK_ARG(k >= 1 && k <= TK_K_MAX, "score_extremes: k must be in [1, %d], not %d", TK_K_MAX, k);
    EOE_CHECK_ARG(((uintptr_t)scratch & 15) == 0 && ((uintptr_t)out_idx & 3) == 0 && ((uintptr_t)out_val & 3) == 0 &&
                      ((uintptr_t)out_counts & 3) == 0,
                  "score_extremes: scratch must be 16-byte aligned, the outputs 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(scratch);
    unsigned* hist = reinterpret_cast<unsigned*>(base + TK_OFF_HIST);
    unsigned* cnt = reinterpret_cast<unsigned*>(base + TK_OFF_CNT);
    TkState* state = reinterpret_cast<TkState*>(base + TK_OFF_STATE);
    unsigned* meta = reinterpret_cast<unsigned*>(base + TK_OFF_META);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + TK_OFF_KEYS);
    const int grid = topk_grid(n);
    ProfScope ps("score_extremes", 0.0, 6.0 * (labels ? 12.0 : 4.0) * (double)n, stream);
    hipError_t e = hipMemsetAsync(base, 0, TK_ZERO_BYTES, st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "score_extremes: clearing the count tables: %s", hipGetErrorString(e));
    for (int p = 0; p < TK_PASSES; ++p) {
        hipLaunchKernelGGL(topk_pass_kernel, dim3(grid), dim3(TK_NT), 0, st, scores, labels, n, k, p, hist, state, meta, cnt + TK_LISTS);
        EOE_CHECK_LAUNCH("score_extremes (digit pass)");
    }
    hipLaunchKernelGGL(topk_gather_kernel, dim3(grid), dim3(TK_NT), 0, st, scores, labels, n, k, (const unsigned*)hist, state, meta, cnt, keys);
    EOE_CHECK_LAUNCH("score_extremes (gather)");
    hipLaunchKernelGGL(topk_sort_kernel, dim3(TK_LISTS), dim3(TK_K_MAX), 0, st, scores, n, k, (const unsigned*)meta, (const unsigned*)cnt,
                       (const unsigned*)(cnt + TK_LISTS), (const unsigned long long*)keys, out_idx, out_val, out_counts);
    EOE_CHECK_LAUNCH("score_extremes (sort)");
    return 0;
}
