// Candidate search of the evolutionary OE-sample experiment (`src/eoe/evolve/__init__.py:100-157`): the reference pulls a pool of
// candidate images through the host dataset one at a time, takes their squared distance to the parent image(s) and sorts.  Here the
// images already sit in HBM as uint8 (ResidentImageSource.oe), so the search is a gather plus a bandwidth-bound distance kernel,
// exact in integers, and a rank-by-counting sort.
//
// eoe_pool_sqdist_u8: out[k][p] = sum_e (set[q_k][e] - set[c_p][e])^2 over the D bytes of an image, exact int64.
//   * One workgroup per (candidate, chunk of D).  The candidate's bytes of the chunk are loaded once (16 bytes per lane and piece,
//     up to 16 pieces per thread kept in registers) and compared against all K queries; the queries come back from L2 (K images).
//   * D is split over workgroups so that the grid fills the chip when P is small (P = 100 at 32 x 32 x 3 is 300 KB in all): the
//     chunk is the multiple of 1 024 bytes that gives about 1 024 workgroups, at least 1 024 bytes (one wave of 16-byte loads), at
//     most 65 536 bytes.  A partial sum over at most 65 536 bytes fits 32 bits (255^2 * 65 536 < 2^32), so a chunk accumulates in
//     32 bits; the chunks are combined in 64 bits.
//   * Combination is a second pass, no atomics: every workgroup stores its K partial sums into the workspace ([K][P][chunks]
//     uint32) and a small kernel adds a pair's chunks in index order (a single chunk is written to `out` directly, one launch).
//     Integer sums would be bit-identical in any order; the second pass needs no zeroed output and costs one tiny launch.
//   * D a multiple of 16 (and a 16-byte aligned set) takes the 16-byte loads; anything else a byte-wise path that re-reads the
//     candidate per query from cache (correct, tested at 7 x 9 x 3, slow for large images), as normstats.hip does.
//   * The index lists are HOST arrays: they are checked against the set before anything is launched and copied into the workspace
//     on the stream; a bad index is an error code, never a dereference.
// eoe_pool_rank: for each of the K rows the stable ascending order of its P distances as int32 positions (the `arg` of the
//   reference's `distances.sort()`); equal distances keep candidate-list order.  One launch, one workgroup per row, rank by counting
//   over the row held in LDS: position p goes to slot #{j : d_j < d_p or (d_j == d_p and j < p)}.  P <= 1 024.
#include "common.h"

namespace {

constexpr int PD_NT = 256;
constexpr int PD_PIECES = 16;                  // 16-byte pieces of the candidate chunk a thread keeps: 16 * 256 * 16 B = 65 536 B
constexpr int PD_CHUNK_MIN = 1024;
constexpr int PD_CHUNK_MAX = PD_PIECES * PD_NT * 16;       // 65 536: 255^2 * 65 536 = 4 261 478 400 < 2^32
constexpr int PD_TARGET_BLOCKS = 1024;
constexpr int PD_K_MAX = 1024;                 // K * 4 partial sums of the waves in LDS (16 KB)
constexpr int PD_P_MAX = 1 << 20;
constexpr int RANK_P_MAX = 1024;
constexpr long long PD_MAX_FEATURES = 1ll << 26;
constexpr size_t PD_ALIGN = 256;

static_assert((long long)255 * 255 * PD_CHUNK_MAX < (1ll << 32), "a chunk's partial sum must fit 32 bits");

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// sum of the four squared byte differences of two dwords
__device__ __forceinline__ unsigned sqdiff4(unsigned a, unsigned b) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((a >> (8 * k)) & 0xffu) - (int)((b >> (8 * k)) & 0xffu);
        s += (unsigned)(d * d);
    }
    return s;
}

// grid: P * nchunks workgroups, block b = candidate b / nchunks, chunk b % nchunks.  qidx / cidx were validated on the host.
__global__ __launch_bounds__(PD_NT) void sqdist_kernel(const uint8_t* __restrict__ set, int D, int chunk, int nchunks,
                                                       const int* __restrict__ qidx, const int* __restrict__ cidx, int K, int P,
                                                       unsigned* __restrict__ part, long long* __restrict__ out, int vec16) {
    __shared__ unsigned red[PD_K_MAX * (PD_NT / 64)];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int p = blockIdx.x / nchunks, c = blockIdx.x - p * nchunks;
    const int begin = c * chunk, len = min(chunk, D - begin);
    const uint8_t* cp = set + (size_t)cidx[p] * D + begin;
    if (vec16) {
        const int npieces = len >> 4;                          // D and chunk are multiples of 16, so is len
        const u32x4* cpv = reinterpret_cast<const u32x4*>(cp);
        u32x4 cv[PD_PIECES];
#pragma unroll
        for (int r = 0; r < PD_PIECES; ++r) {
            const int i = t + r * PD_NT;
            cv[r] = i < npieces ? cpv[i] : u32x4{0u, 0u, 0u, 0u};
        }
        for (int k = 0; k < K; ++k) {
            const u32x4* qpv = reinterpret_cast<const u32x4*>(set + (size_t)qidx[k] * D + begin);
            unsigned acc = 0;
#pragma unroll
            for (int r = 0; r < PD_PIECES; ++r) {
                const int i = t + r * PD_NT;
                if (i < npieces) {
                    const u32x4 q = qpv[i];
                    acc += sqdiff4(q[0], cv[r][0]) + sqdiff4(q[1], cv[r][1]) + sqdiff4(q[2], cv[r][2]) + sqdiff4(q[3], cv[r][3]);
                }
            }
            acc = wave_sum_u32(acc);
            if (lane == 0) red[k * (PD_NT / 64) + wave] = acc;
        }
    } else {
        for (int k = 0; k < K; ++k) {
            const uint8_t* qp = set + (size_t)qidx[k] * D + begin;
            unsigned acc = 0;
            for (int j = t; j < len; j += PD_NT) {
                const int d = (int)cp[j] - (int)qp[j];
                acc += (unsigned)(d * d);
            }
            acc = wave_sum_u32(acc);
            if (lane == 0) red[k * (PD_NT / 64) + wave] = acc;
        }
    }
    __syncthreads();
    for (int k = t; k < K; k += PD_NT) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < PD_NT / 64; ++w) s += red[k * (PD_NT / 64) + w];
        const size_t o = (size_t)k * P + p;
        if (nchunks == 1) out[o] = (long long)s;
        else part[o * nchunks + c] = s;
    }
}

__global__ __launch_bounds__(PD_NT) void combine_kernel(const unsigned* __restrict__ part, int nchunks, long long pairs,
                                                        long long* __restrict__ out) {
    const long long o = (long long)blockIdx.x * PD_NT + threadIdx.x;
    if (o >= pairs) return;
    const unsigned* pp = part + (size_t)o * nchunks;
    unsigned long long s = 0;
    for (int c = 0; c < nchunks; ++c) s += pp[c];
    out[o] = (long long)s;
}

__global__ __launch_bounds__(PD_NT) void rank_kernel(const long long* __restrict__ dist, int P, int* __restrict__ order) {
    __shared__ long long d[RANK_P_MAX];
    const int t = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * P;
    for (int j = t; j < P; j += PD_NT) d[j] = dist[row + j];
    __syncthreads();
    for (int p = t; p < P; p += PD_NT) {
        const long long v = d[p];
        int r = 0;
        for (int j = 0; j < P; ++j) r += (d[j] < v || (d[j] == v && j < p)) ? 1 : 0;       // every lane reads the same word
        order[row + r] = p;
    }
}

int pick_chunk(long long D, int P) {
    const long long want = (PD_TARGET_BLOCKS + P - 1) / P;                   // chunks per candidate for a full grid
    long long chunk = (D + want - 1) / want;
    chunk = (chunk + PD_CHUNK_MIN - 1) / PD_CHUNK_MIN * PD_CHUNK_MIN;
    if (chunk > PD_CHUNK_MAX) chunk = PD_CHUNK_MAX;
    return (int)chunk;
}

size_t index_bytes(int K, int P) { return ((size_t)(K + P) * sizeof(int32_t) + PD_ALIGN - 1) / PD_ALIGN * PD_ALIGN; }

int check_shape(const char* who, int64_t D, int K, int P) {
    EOE_CHECK_ARG(D > 0 && D <= PD_MAX_FEATURES, "%s: images of 1 to %lld bytes, not %lld", who, PD_MAX_FEATURES, (long long)D);
    EOE_CHECK_ARG(K >= 1 && K <= PD_K_MAX, "%s: K (queries) must be in [1, %d], not %d", who, PD_K_MAX, K);
    EOE_CHECK_ARG(P >= 1 && P <= PD_P_MAX, "%s: P (candidates) must be in [1, %d], not %d", who, PD_P_MAX, P);
    return 0;
}

}  // namespace

extern "C" int eoe_pool_sqdist_workspace(int64_t D, int K, int P, size_t* bytes_out) {
    EOE_CHECK_ARG(bytes_out, "pool_sqdist_workspace: null bytes_out");
    EOE_TRY(check_shape("pool_sqdist_workspace", D, K, P));
    const int chunk = pick_chunk(D, P);
    const long long nchunks = (D + chunk - 1) / chunk;
    *bytes_out = index_bytes(K, P) + (nchunks > 1 ? (size_t)K * P * nchunks * sizeof(uint32_t) : 0);
    return 0;
}

extern "C" int eoe_pool_sqdist_u8(const uint8_t* set, int64_t n_set, int64_t D, const int32_t* query_idx, int K,
                                  const int32_t* cand_idx, int P, int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    EOE_CHECK_ARG(set && query_idx && cand_idx && out && workspace, "pool_sqdist_u8: null image set, index list, output or workspace");
    EOE_CHECK_ARG(n_set > 0 && n_set < (1ll << 31), "pool_sqdist_u8: n_set must be in [1, 2^31), not %lld", (long long)n_set);
    EOE_TRY(check_shape("pool_sqdist_u8", D, K, P));
    for (int k = 0; k < K; ++k)
        EOE_CHECK_ARG(query_idx[k] >= 0 && query_idx[k] < n_set, "pool_sqdist_u8: query %d is row %d, outside the set of %lld rows", k,
                      query_idx[k], (long long)n_set);
    for (int p = 0; p < P; ++p)
        EOE_CHECK_ARG(cand_idx[p] >= 0 && cand_idx[p] < n_set, "pool_sqdist_u8: candidate %d is row %d, outside the set of %lld rows", p,
                      cand_idx[p], (long long)n_set);
    const int chunk = pick_chunk(D, P);
    const long long nchunks = (D + chunk - 1) / chunk, blocks = nchunks * P, pairs = (long long)K * P;
    EOE_CHECK_ARG(blocks < (1ll << 31), "pool_sqdist_u8: %d candidates x %lld chunks exceed the grid", P, nchunks);
    size_t need = 0;
    EOE_TRY(eoe_pool_sqdist_workspace(D, K, P, &need));
    EOE_CHECK_ARG(workspace_bytes >= need, "pool_sqdist_u8: workspace of %zu bytes, %zu needed (eoe_pool_sqdist_workspace)", workspace_bytes,
                  need);
    EOE_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 7) == 0, "pool_sqdist_u8: workspace must be 16-byte and out 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int* qidx = static_cast<int*>(workspace);
    int* cidx = qidx + K;
    unsigned* part = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + index_bytes(K, P));
    hipError_t e = hipMemcpyAsync(qidx, query_idx, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cidx, cand_idx, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "pool_sqdist_u8: index copy: %s", hipGetErrorString(e));
    const int vec16 = (D % 16 == 0) && (((uintptr_t)set & 15) == 0);
    ProfScope ps("pool_sqdist_u8", 3.0 * (double)D * (double)pairs, (double)D * (double)(P + K) + 8.0 * (double)pairs, stream);
    hipLaunchKernelGGL(sqdist_kernel, dim3((unsigned)blocks), dim3(PD_NT), 0, st, set, (int)D, chunk, (int)nchunks, (const int*)qidx,
                       (const int*)cidx, K, P, part, (long long*)out, vec16);
    EOE_CHECK_LAUNCH("pool_sqdist_u8");
    if (nchunks > 1) {
        hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((pairs + PD_NT - 1) / PD_NT)), dim3(PD_NT), 0, st, (const unsigned*)part,
                           (int)nchunks, pairs, (long long*)out);
        EOE_CHECK_LAUNCH("pool_sqdist_u8 (combine)");
    }
    return 0;
}

extern "C" int eoe_pool_rank(const int64_t* dist, int K, int P, int32_t* order, void* stream) {
    EOE_CHECK_ARG(dist && order, "pool_rank: null distances or output");
    EOE_CHECK_ARG(K >= 1 && K <= PD_K_MAX, "pool_rank: K (rows) must be in [1, %d], not %d", PD_K_MAX, K);
    EOE_CHECK_ARG(P >= 1, "pool_rank: P (candidates) must be positive, not %d", P);
    if (P > RANK_P_MAX) return eoe_set_error(EOE_ERR_UNSUPPORTED, "pool_rank: rows of at most %d distances, not %d", RANK_P_MAX, P);
    ProfScope ps("pool_rank", 0, 12.0 * (double)K * (double)P, stream);
    hipLaunchKernelGGL(rank_kernel, dim3((unsigned)K), dim3(PD_NT), 0, (hipStream_t)stream, (const long long*)dist, P, (int*)order);
    EOE_CHECK_LAUNCH("pool_rank");
    return 0;
}
