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
// eoe_pool_sqdist_ragged_u8: the same sum over a crop_h x crop_w x C WINDOW of every listed image of a set of mixed sizes (arena,
//   offsets, sizes as in augment.hip), each given as (row, top, left) relative to its own unpadded image; window bytes outside the
//   image count as 0 (CenterCrop's zero padding).  The window is numbered in its OWN packed layout, e = (y * crop_w + x) * C + c, and
//   split into chunks and pieces of 16 bytes exactly as above (one workgroup per (candidate, chunk), 32-bit partial sums, the same
//   second pass).  What differs is how a piece is fetched: window rows are not aligned (W * C and left * C are arbitrary, and a query
//   and a candidate are misaligned differently), so a piece that lies in one window row and wholly inside the image is read as the
//   4 or 5 ALIGNED dwords that cover it and shifted into place (v_alignbyte); the candidate's pieces are packed once and kept in
//   registers for all K queries, a query's pieces are packed the same way, and dwords are compared with dwords.  Any other piece
//   (it crosses a window row, or the image's edge, or the window's end) is put together byte by byte with every byte bounds-checked.
//   No load leaves [arena, arena + arena_bytes): the aligned reads start at or after the arena's start (a multiple of 16) and a
//   covering dword holds at least one byte of the image, so it ends inside the arena, whose length is a multiple of 16; an image
//   whose extent in the device tables does not lie in the arena is treated as empty.
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

// the workgroup's K sums (one per wave in `red`) -> the pair's slot of chunk c in the workspace, or `out` itself when there is one chunk
__device__ __forceinline__ void store_partials(const unsigned* red, int K, int P, int p, int c, int nchunks, unsigned* __restrict__ part,
                                               long long* __restrict__ out) {
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += PD_NT) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < PD_NT / 64; ++w) s += red[k * (PD_NT / 64) + w];
        const size_t o = (size_t)k * P + p;
        if (nchunks == 1) out[o] = (long long)s;
        else part[o * nchunks + c] = s;
    }
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
    store_partials(red, K, P, p, c, nchunks, part, out);
}

// ------------------------------------------------------------------------------------------------------------ ragged windows
// one listed image as the workgroup sees it: where it starts in the arena, its rows, its row length in bytes and the window's origin in
// rows and bytes.  An image the arena does not hold has H = 0 (every row test fails: all zeros).  The origin is clamped to
// [-crop, extent]: beyond that the window is wholly outside either way, and the sums below stay far inside 32 bits.
struct Window {
    size_t at;
    int H, WC, top, leftb;
};

__device__ __forceinline__ Window window_of(long long arena_bytes, const long long* __restrict__ offsets, const int* __restrict__ sizes,
                                            const int* __restrict__ d, int C, int crop_h, int crop_w) {
    const int row = d[0];
    const long long off = offsets[row];
    const int H = sizes[2 * row], W = sizes[2 * row + 1];
    const bool held = H > 0 && W > 0 && (long long)W * C < (1ll << 30) && off >= 0 && off <= arena_bytes &&
                      (long long)H * ((long long)W * C) <= arena_bytes - off;
    Window w;
    w.at = held ? (size_t)off : 0;
    w.H = held ? H : 0;
    w.WC = held ? W * C : 0;
    w.top = max(-crop_h, min(d[1], w.H));
    w.leftb = max(-crop_w, min(d[2], held ? W : 0)) * C;
    return w;
}

// 16 bytes of the window from element e = y * rowb + xb on, byte by byte: rows and columns outside the image and elements past the
// window's end are 0.  The rare path (a piece that crosses a window row or an edge): a call, not 32 inlined copies in the kernel.
__device__ __noinline__ u32x4 gather16_bytes(const uint8_t* __restrict__ arena, Window w, int y, int xb, int e, int Dw, int rowb) {
    u32x4 v;
    for (int j = 0; j < 4; ++j) {
        unsigned word = 0;
        for (int b = 0; b < 4; ++b, ++e) {
            const int r = y + w.top, cb = w.leftb + xb;
            if (e < Dw && r >= 0 && r < w.H && cb >= 0 && cb < w.WC) word |= (unsigned)arena[w.at + (size_t)r * w.WC + cb] << (8 * b);
            if (++xb == rowb) xb = 0, ++y;
        }
        v[j] = word;
    }
    return v;
}

// 16 bytes of the window in its packed layout.  A piece inside one window row and inside the image: the aligned dwords that cover
// it (a fifth one only when it does not start on a dword), shifted into place.
__device__ __forceinline__ u32x4 gather16(const uint8_t* __restrict__ arena, const Window& w, int y, int xb, int e, int Dw, int rowb) {
    const int r = y + w.top, cb = w.leftb + xb;
    if (xb + 16 <= rowb) {                                     // one window row (and so e + 16 <= Dw)
        if (r < 0 || r >= w.H || cb + 16 <= 0 || cb >= w.WC) return u32x4{0u, 0u, 0u, 0u};
        if (cb >= 0 && cb + 16 <= w.WC) {
            const size_t a = w.at + (size_t)r * w.WC + cb;
            const unsigned sh = (unsigned)(a & 3);
            const unsigned* src = reinterpret_cast<const unsigned*>(arena + (a - sh));
            const unsigned d0 = src[0], d1 = src[1], d2 = src[2], d3 = src[3], d4 = sh ? src[4] : 0u;
            return u32x4{__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                         __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
        }
    }
    return gather16_bytes(arena, w, y, xb, e, Dw, rowb);
}

// grid and partial sums as sqdist_kernel; desc = (row, top, left) of the K queries, then of the P candidates (rows validated on the host)
__global__ __launch_bounds__(PD_NT) void sqdist_ragged_kernel(const uint8_t* __restrict__ arena, long long arena_bytes,
                                                              const long long* __restrict__ offsets, const int* __restrict__ sizes,
                                                              int C, int crop_h, int crop_w, int Dw, int chunk, int nchunks,
                                                              const int* __restrict__ desc, int K, int P, unsigned* __restrict__ part,
                                                              long long* __restrict__ out) {
    __shared__ unsigned red[PD_K_MAX * (PD_NT / 64)];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int p = blockIdx.x / nchunks, c = blockIdx.x - p * nchunks;
    const int begin = c * chunk, len = min(chunk, Dw - begin), rowb = crop_w * C;
    const int npieces = (len + 15) >> 4;                       // the window's last piece may be short: its tail reads as 0 on both sides
    const Window cw = window_of(arena_bytes, offsets, sizes, desc + 3 * (K + p), C, crop_h, crop_w);
    u32x4 cv[PD_PIECES];
    int py[PD_PIECES], px[PD_PIECES];                          // window row and byte in that row of each piece: the same for every image
#pragma unroll
    for (int r = 0; r < PD_PIECES; ++r) {
        const int i = t + r * PD_NT, e = begin + 16 * i;
        py[r] = e / rowb;
        px[r] = e - py[r] * rowb;
        cv[r] = i < npieces ? gather16(arena, cw, py[r], px[r], e, Dw, rowb) : u32x4{0u, 0u, 0u, 0u};
    }
    for (int k = 0; k < K; ++k) {
        const Window qw = window_of(arena_bytes, offsets, sizes, desc + 3 * k, C, crop_h, crop_w);
        unsigned acc = 0;
#pragma unroll
        for (int r = 0; r < PD_PIECES; ++r) {
            const int i = t + r * PD_NT;
            if (i < npieces) {
                const u32x4 q = gather16(arena, qw, py[r], px[r], begin + 16 * i, Dw, rowb);
                acc += sqdiff4(q[0], cv[r][0]) + sqdiff4(q[1], cv[r][1]) + sqdiff4(q[2], cv[r][2]) + sqdiff4(q[3], cv[r][3]);
            }
        }
        acc = wave_sum_u32(acc);
        if (lane == 0) red[k * (PD_NT / 64) + wave] = acc;
    }
    store_partials(red, K, P, p, c, nchunks, part, out);
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

size_t desc_bytes(int K, int P) { return ((size_t)(K + P) * 3 * sizeof(int32_t) + PD_ALIGN - 1) / PD_ALIGN * PD_ALIGN; }

// the window's bytes, or an error: each side and the product are held to PD_MAX_FEATURES, so nothing here can overflow
int window_bytes(const char* who, int crop_h, int crop_w, int C, int64_t* Dw) {
    EOE_CHECK_ARG(C == 1 || C == 3, "%s: C must be 1 or 3, not %d", who, C);
    EOE_CHECK_ARG(crop_h >= 0 && crop_w >= 0 && crop_h <= PD_MAX_FEATURES && crop_w <= PD_MAX_FEATURES, "%s: a window of %d x %d", who,
                  crop_h, crop_w);
    const long long px = (long long)crop_h * crop_w;
    *Dw = px > PD_MAX_FEATURES ? PD_MAX_FEATURES + 1 : px * C;
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

extern "C" int eoe_pool_sqdist_ragged_workspace(int crop_h, int crop_w, int C, int K, int P, size_t* bytes_out) {
    EOE_CHECK_ARG(bytes_out, "pool_sqdist_ragged_workspace: null bytes_out");
    int64_t Dw = 0;
    EOE_TRY(window_bytes("pool_sqdist_ragged_workspace", crop_h, crop_w, C, &Dw));
    EOE_TRY(check_shape("pool_sqdist_ragged_workspace", Dw, K, P));
    const int chunk = pick_chunk(Dw, P);
    const long long nchunks = (Dw + chunk - 1) / chunk;
    *bytes_out = desc_bytes(K, P) + (nchunks > 1 ? (size_t)K * P * nchunks * sizeof(uint32_t) : 0);
    return 0;
}

extern "C" int eoe_pool_sqdist_ragged_u8(const uint8_t* arena, int64_t arena_bytes, const int64_t* offsets, const int32_t* sizes,
                                         int64_t n_set, int C, int crop_h, int crop_w, const int32_t* query, int K, const int32_t* cand,
                                         int P, int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pool_sqdist_ragged_u8";
    EOE_CHECK_ARG(arena && offsets && sizes && query && cand && out && workspace,
                  "%s: null arena, offsets, sizes, window list, output or workspace", who);
    EOE_CHECK_ARG(n_set > 0 && n_set < (1ll << 31), "%s: n_set must be in [1, 2^31), not %lld", who, (long long)n_set);
    EOE_CHECK_ARG(arena_bytes > 0 && arena_bytes % 16 == 0 && ((uintptr_t)arena & 15) == 0,
                  "%s: the arena must start at and be as long as a multiple of 16 bytes (%lld bytes given)", who, (long long)arena_bytes);
    int64_t Dw = 0;
    EOE_TRY(window_bytes(who, crop_h, crop_w, C, &Dw));
    EOE_TRY(check_shape(who, Dw, K, P));
    for (int k = 0; k < K; ++k)
        EOE_CHECK_ARG(query[3 * k] >= 0 && query[3 * k] < n_set, "%s: query %d is row %d, outside the set of %lld rows", who, k,
                      query[3 * k], (long long)n_set);
    for (int p = 0; p < P; ++p)
        EOE_CHECK_ARG(cand[3 * p] >= 0 && cand[3 * p] < n_set, "%s: candidate %d is row %d, outside the set of %lld rows", who, p,
                      cand[3 * p], (long long)n_set);
    const int chunk = pick_chunk(Dw, P);
    const long long nchunks = (Dw + chunk - 1) / chunk, blocks = nchunks * P, pairs = (long long)K * P;
    EOE_CHECK_ARG(blocks < (1ll << 31), "%s: %d candidates x %lld chunks exceed the grid", who, P, nchunks);
    size_t need = 0;
    EOE_TRY(eoe_pool_sqdist_ragged_workspace(crop_h, crop_w, C, K, P, &need));
    EOE_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed (eoe_pool_sqdist_ragged_workspace)", who, workspace_bytes,
                  need);
    EOE_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 7) == 0, "%s: workspace must be 16-byte and out 8-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    int* desc = static_cast<int*>(workspace);
    unsigned* part = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + desc_bytes(K, P));
    // two lists that lie back to back on the host (OEPool builds them so) go up in one copy
    const bool joined = cand == query + 3 * (size_t)K;
    hipError_t e = hipMemcpyAsync(desc, query, (size_t)(joined ? K + P : K) * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !joined) e = hipMemcpyAsync(desc + 3 * K, cand, (size_t)P * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "%s: window list copy: %s", who, hipGetErrorString(e));
    ProfScope ps(who, 3.0 * (double)Dw * (double)pairs, (double)Dw * (double)(P + K) + 8.0 * (double)pairs, stream);
    hipLaunchKernelGGL(sqdist_ragged_kernel, dim3((unsigned)blocks), dim3(PD_NT), 0, st, arena, (long long)arena_bytes,
                       (const long long*)offsets, (const int*)sizes, C, crop_h, crop_w, (int)Dw, chunk, (int)nchunks, (const int*)desc, K, P,
                       part, (long long*)out);
    EOE_CHECK_LAUNCH(who);
    if (nchunks > 1) {
        hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((pairs + PD_NT - 1) / PD_NT)), dim3(PD_NT), 0, st, (const unsigned*)part,
                           (int)nchunks, pairs, (long long*)out);
        EOE_CHECK_LAUNCH("pool_sqdist_ragged_u8 (combine)");
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
