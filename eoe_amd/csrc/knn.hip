// Nearest neighbours between two sets of fp32 feature vectors: for every query row the k reference rows with the smallest squared
// Euclidean distance, ascending by distance, equal distances by ascending reference index -- np.argsort(d2_row, kind="stable")[:k].
// The nq x nr distance matrix is never written: a workgroup forms a 128 x 128 tile of it on the fp32 matrix cores and reduces it to
// per-query candidate lists in LDS at once.
//
//   norms         one wave per row of q and of r: the sum of squares (an fmaf chain per lane, then a wave sum) and a flag for a row
//                 that holds a NaN or an infinity, both written with ordinary stores.
//   distances     d2 = (|q|^2 + |r|^2) - 2 q.r, clamped at 0.  The dot products run on v_mfma_f32_32x32x2_f32: fp32 in, fp32
//                 accumulate, bit for bit a k-ordered fmaf chain (no 16-bit rounding enters a ranking).  A = references, B = queries,
//                 so a lane of the result holds ONE query and 16 references: the tile goes to LDS as [reference][query] with the
//                 query contiguous, free of bank conflicts on the way in and on the way out.
//   tile          the 128 references x 128 queries x 32 tile layer of f32_tile.h (its workgroup shape, operand images of stride 129,
//                 k order and accumulator map).  The next k-step's global loads are issued in front of the MFMAs of this one.
//   LDS           65 536 B (the distance tile; the operand tiles, 33 024 B, alias it) + 1 024 B (the tile's reference norms and
//                 flags) + k * 8 B * 256 lists (k <= 32) or * 128 lists (k > 32): 76.8 KB at k = 5 (2 workgroups = 2 waves per SIMD),
//                 132 KB at k = 64 (1 wave per SIMD; the fp32 MFMA reaches its rate from one wave with four accumulators).
//   select        a workgroup takes 128 queries and one chunk of 1 024 references (8 tiles).  After a tile, one thread (k > 32) or
//                 two threads (each half of the tile's references) per query walk its distances in ascending reference order and keep
//                 the k smallest keys seen, key = ordered_bits(d2) << 32 | reference index (the order-preserving image topk.hip uses), in a
//                 sorted list in LDS ([slot][thread]: lanes of a wave hit consecutive banks); the k-th key stays in a register, so a
//                 candidate costs one compare unless it enters.  At the chunk's end the two lists of a query are merged and the k keys go
//                 to scratch[nq][chunks][k] (an empty slot is all ones).
//   merge         one wave per query: k rounds of "the smallest key above the last one" over its chunks * k keys, which are distinct,
//                 then index and distance from the key.  Wave 0 also adds up the row flags into counts.
// Integer compares only once a distance is formed, no atomics, every scratch word that is read is written first: two runs give the
// same bytes and a dirty scratch changes nothing.  Three launches on the caller's stream.
#include "f32_tile.h"

namespace {

using namespace f32_tile;

constexpr int KN_NT = NT;
constexpr int KN_BM = TILE;                    // queries per workgroup
constexpr int KN_BN = TILE;                    // references per tile
constexpr int KN_LD = LD_QUAD;                 // a 16-byte load holds four k of one row: transposing stores
constexpr int KN_CHUNK = 1024;                 // references per workgroup
constexpr int KN_K_MAX = 64;
constexpr int KN_D_MAX = 2048;
constexpr int KN_NR_MAX = 1 << 24;
constexpr unsigned long long KN_EMPTY = ~0ull;
constexpr unsigned KN_INF_BITS = 0xFF800000u;  // ordered_bits(+inf): every eligible distance is at or below it

int knn_chunks(int nr) { return cdiv(nr, KN_CHUNK); }
__host__ __device__ constexpr int knn_tpr(int k) { return k <= 32 ? 2 : 1; }           // selection threads per query
size_t knn_lds_bytes(int k) { return (size_t)KN_BN * KN_BM * 4 + (size_t)k * KN_BM * knn_tpr(k) * 8; }

struct KnnScratch {                            // byte offsets into the caller's scratch
    size_t qn, rn, qf, rf, keys, total;
};
KnnScratch knn_layout(int nq, int nr, int k) {
    KnnScratch s;
    s.qn = 0;
    s.rn = s.qn + align_up((size_t)nq * 4, 16);
    s.qf = s.rn + align_up((size_t)nr * 4, 16);
    s.rf = s.qf + align_up((size_t)nq * 4, 16);
    s.keys = s.rf + align_up((size_t)nr * 4, 16);
    s.total = s.keys + align_up((size_t)nq * knn_chunks(nr) * k * 8, 16) + 16;
    return s;
}

// one wave per row of q (rows [0, nq)) and of r (rows [nq, nq + nr)): squared norm and the non-finite flag
__global__ __launch_bounds__(KN_NT) void knn_norm_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ r, int ldr, int nq,
                                                         int nr, int D, float* __restrict__ qn, float* __restrict__ rn, int* __restrict__ qf,
                                                         int* __restrict__ rf) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (KN_NT / 64) + (threadIdx.x >> 6);
    if (row >= (long long)nq + nr) return;
    const bool isq = row < nq;
    const int i = isq ? (int)row : (int)(row - nq);
    const float* p = isq ? q + (size_t)i * ldq : r + (size_t)i * ldr;
    float s = 0.f;
    const bool any = row_nonfinite(p, D, lane, [&](float v) { s = fmaf(v, v, s); });
    s = wave_sum(s);
    if (lane == 0) {
        (isq ? qn : rn)[i] = s;
        (isq ? qf : rf)[i] = any ? 1 : 0;
    }
}

// keeps the k smallest keys in the sorted list L[slot * stride]; thr is its last slot
__device__ __forceinline__ void knn_insert(unsigned long long* __restrict__ L, int stride, int k, unsigned long long key,
                                           unsigned long long& thr) {
    int s = k - 1;
    while (s > 0) {
        const unsigned long long p = L[(s - 1) * stride];
        if (p <= key) break;
        L[s * stride] = p;
        --s;
    }
    L[s * stride] = key;
    thr = L[(k - 1) * stride];
}

__global__ __launch_bounds__(KN_NT) void knn_tile_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ r, int ldr, int nq,
                                                         int nr, int D, int k, int chunks, int vecq, int vecr,
                                                         const float* __restrict__ qnorm, const float* __restrict__ rnorm,
                                                         const int* __restrict__ rflag, unsigned long long* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) char kn_lds[];
    __shared__ float rn_s[KN_BN];
    __shared__ int rok_s[KN_BN];
    float* stage = reinterpret_cast<float*>(kn_lds);                          // [KN_BN references][KN_BM queries]
    float* As = stage;                                                        // [BK][KN_LD] references, aliases the stage
    float* Bs = stage + BK * KN_LD;                                           // [BK][KN_LD] queries
    unsigned long long* lists = reinterpret_cast<unsigned long long*>(kn_lds + (size_t)KN_BN * KN_BM * 4);

    const int t = threadIdx.x;
    const Wave w = wave_coords();                                             // the wave's 64 references (A) x 64 queries (B) of the tile
    const int ch = (int)(blockIdx.x % (unsigned)chunks), qb = (int)(blockIdx.x / (unsigned)chunks);
    const int q0 = qb * KN_BM;
    const int tpr = knn_tpr(k), nsel = KN_BM * tpr, per = KN_BN / tpr;
    const int lk = (t & 7) * 4, lrow = t >> 3;                                // loads: k quad and first row (then + 32)

    unsigned long long thr = KN_EMPTY;
    unsigned long long* mine = lists + t;
    if (t < nsel)
        for (int s = 0; s < k; ++s) mine[s * nsel] = KN_EMPTY;

    float qn[2];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        const int qq = q0 + b_row(w, qi);
        qn[qi] = qq < nq ? qnorm[qq] : 0.f;
    }

    const int nkt = (D + BK - 1) / BK;
    for (int tile = 0; tile < KN_CHUNK / KN_BN; ++tile) {
        const int r0 = ch * KN_CHUNK + tile * KN_BN;
        if (r0 >= nr) break;                                                  // uniform over the workgroup
        Acc acc;
        zero(acc);
        float4 ra[4], rb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                         // a row past its set reads as zeros
            ra[j] = load_quad(r, ldr, r0 + lrow + 32 * j, lk, D, vecr != 0, r0 + lrow + 32 * j < nr);
            rb[j] = load_quad(q, ldq, q0 + lrow + 32 * j, lk, D, vecq != 0, q0 + lrow + 32 * j < nq);
        }
        for (int kt = 0; kt < nkt; ++kt) {
            __syncthreads();                                                  // the last reads of the operand tiles and of the stage are done
            if (kt == 0 && t < KN_BN) {
                const int rr = r0 + t;
                rn_s[t] = rr < nr ? rnorm[rr] : 0.f;
                rok_s[t] = rr < nr ? (rflag[rr] == 0) : 0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                store_quad_t<KN_LD>(As, lk, lrow + 32 * j, ra[j]);
                store_quad_t<KN_LD>(Bs, lk, lrow + 32 * j, rb[j]);
            }
            __syncthreads();
            if (kt + 1 < nkt) {
                const int kk = (kt + 1) * BK + lk;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ra[j] = load_quad(r, ldr, r0 + lrow + 32 * j, kk, D, vecr != 0, r0 + lrow + 32 * j < nr);
                    rb[j] = load_quad(q, ldq, q0 + lrow + 32 * j, kk, D, vecq != 0, q0 + lrow + 32 * j < nq);
                }
            }
            mma_step<KN_LD>(As, Bs, acc, w);
        }
        __syncthreads();                                                      // every wave has read its operands: the stage may take their place
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)                                        // acc_walk's order, spelled out: see the note at acc_walk
#pragma unroll
            for (int qi = 0; qi < 2; ++qi)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int rl = a_row(w, ri, e), ql = b_row(w, qi);
                    stage[rl * KN_BM + ql] = fmaf(-2.f, acc[ri][qi][e], qn[qi] + rn_s[rl]);
                }
        __syncthreads();
        if (t < nsel) {
            const int ql = t & (KN_BM - 1), c0 = (t >> 7) * per;
            for (int c = c0; c < c0 + per; ++c) {
                if (!rok_s[c]) continue;                                      // past the set or a non-finite row: never a candidate
                float d = stage[c * KN_BM + ql];
                if (!(d > 0.f)) d = (d != d) ? __uint_as_float(0x7F800000u) : 0.f;      // clamp at 0; inf - inf of finite rows counts as inf
                const unsigned long long key = ((unsigned long long)ordered_bits(d) << 32) | (unsigned)(r0 + c);
                if (key < thr && (unsigned)(key >> 32) <= KN_INF_BITS) knn_insert(mine, nsel, k, key, thr);
            }
        }
    }
    __syncthreads();
    if (t < KN_BM) {
        if (tpr == 2) {
            const unsigned long long* other = lists + t + KN_BM;
            for (int s = 0; s < k; ++s) {
                const unsigned long long key = other[s * nsel];
                if (key >= thr) break;                                        // the partner's list is ascending
                knn_insert(mine, nsel, k, key, thr);
            }
        }
        const int qq = q0 + t;
        if (qq < nq) {
            unsigned long long* out = keys + ((size_t)qq * chunks + ch) * k;
            for (int s = 0; s < k; ++s) out[s] = mine[s * nsel];
        }
    }
}

// one wave per query: the k smallest of its chunks * k distinct keys, ascending; wave 0 adds up the flags
__global__ __launch_bounds__(64) void knn_merge_kernel(const unsigned long long* __restrict__ keys, int nq, int nr, int k, int chunks,
                                                       const int* __restrict__ qflag, const int* __restrict__ rflag, int* __restrict__ idx,
                                                       float* __restrict__ d2, int* __restrict__ counts) {
    const int qq = blockIdx.x, lane = threadIdx.x;
    if (qq == 0) {
        int cq = 0, cr = 0;
        for (int i = lane; i < nq; i += 64) cq += qflag[i];
        for (int i = lane; i < nr; i += 64) cr += rflag[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cq += __shfl_xor(cq, o, 64);
            cr += __shfl_xor(cr, o, 64);
        }
        if (lane == 0) { counts[0] = cq; counts[1] = cr; }
    }
    int* oi = idx + (size_t)qq * k;
    float* od = d2 + (size_t)qq * k;
    if (qflag[qq]) {
        for (int s = lane; s < k; s += 64) { oi[s] = -1; od[s] = __uint_as_float(0x7FC00000u); }
        return;
    }
    const unsigned long long* mk = keys + (size_t)qq * chunks * k;
    const long long M = (long long)chunks * k;
    unsigned long long prev = 0ull;
    int s = 0;
    for (; s < k; ++s) {
        unsigned long long best = KN_EMPTY;
        for (long long i = lane; i < M; i += 64) {
            const unsigned long long key = mk[i];
            if ((s == 0 || key > prev) && key < best) best = key;
        }
        best = wave_min_u64(best);
        if (best == KN_EMPTY) break;
        if (lane == 0) {
            oi[s] = (int)(unsigned)(best & 0xFFFFFFFFull);
            od[s] = from_ordered_bits((unsigned)(best >> 32));
        }
        prev = best;
    }
    for (int j = s + lane; j < k; j += 64) { oi[j] = -1; od[j] = __uint_as_float(0x7F800000u); }
}

bool knn_in_range(int nq, int nr, int D, int k) {
    return nq >= 0 && nr >= 0 && nr < KN_NR_MAX && D >= 1 && D <= KN_D_MAX && k >= 1 && k <= KN_K_MAX;
}

}  // namespace

extern "C" size_t eoe_feature_knn_scratch_bytes(int nq, int nr, int D, int k) {
    return knn_in_range(nq, nr, D, k) ? knn_layout(nq, nr, k).total : 0;
}

extern "C" int eoe_feature_knn(const float* q, int ldq, const float* r, int ldr, int nq, int nr, int D, int k, int* idx, float* d2, int* counts,
                               void* scratch, void* stream) {
    EOE_CHECK_ARG(q && r && idx && d2 && counts && scratch, "feature_knn: null q, r, idx, d2, counts or scratch");
    EOE_CHECK_ARG(k >= 1 && k <= KN_K_MAX, "feature_knn: k must be in [1, %d], not %d", KN_K_MAX, k);
    EOE_CHECK_ARG(D >= 1 && D <= KN_D_MAX, "feature_knn: D must be in [1, %d], not %d", KN_D_MAX, D);
    EOE_CHECK_ARG(ldq >= D, "feature_knn: ldq must be at least D = %d, not %d", D, ldq);
    EOE_CHECK_ARG(ldr >= D, "feature_knn: ldr must be at least D = %d, not %d", D, ldr);
    EOE_CHECK_ARG(nq >= 0, "feature_knn: nq must not be negative (%d)", nq);
    EOE_CHECK_ARG(nr >= 0 && nr < KN_NR_MAX, "feature_knn: nr must be in [0, 2^24), not %d", nr);
    EOE_CHECK_ARG(((uintptr_t)q & 3) == 0 && ((uintptr_t)r & 3) == 0 && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)d2 & 3) == 0 &&
                      ((uintptr_t)counts & 3) == 0 && ((uintptr_t)scratch & 15) == 0,
                  "feature_knn: q, r, idx, d2 and counts must be 4-byte aligned, scratch 16-byte aligned");
    const int chunks = knn_chunks(nr);
    const long long blocks = (long long)cdiv(nq, KN_BM) * chunks;
    EOE_CHECK_ARG(blocks < (1ll << 31) && (long long)nq + nr < (1ll << 31), "feature_knn: nq = %d with nr = %d is more than one launch covers", nq, nr);
    if (nq == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const KnnScratch lay = knn_layout(nq, nr, k);
    char* base = static_cast<char*>(scratch);
    float* qn = reinterpret_cast<float*>(base + lay.qn);
    float* rn = reinterpret_cast<float*>(base + lay.rn);
    int* qf = reinterpret_cast<int*>(base + lay.qf);
    int* rf = reinterpret_cast<int*>(base + lay.rf);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + lay.keys);
    ProfScope ps("feature_knn", 2.0 * nq * (double)nr * D, 4.0 * ((double)nq + nr) * D, stream);
    const long long rows = (long long)nq + nr;
    hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)((rows + KN_NT / 64 - 1) / (KN_NT / 64))), dim3(KN_NT), 0, st, q, ldq, r, ldr, nq, nr, D,
                       qn, rn, qf, rf);
    EOE_CHECK_LAUNCH("feature_knn (norms)");
    if (chunks > 0) {
        static bool once = (hipFuncSetAttribute((const void*)knn_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)knn_lds_bytes(KN_K_MAX)), true);
        (void)once;
        const int vecq = ((uintptr_t)q & 15) == 0 && (ldq & 3) == 0, vecr = ((uintptr_t)r & 15) == 0 && (ldr & 3) == 0;
        hipLaunchKernelGGL(knn_tile_kernel, dim3((unsigned)blocks), dim3(KN_NT), knn_lds_bytes(k), st, q, ldq, r, ldr, nq, nr, D, k, chunks,
                           vecq, vecr, (const float*)qn, (const float*)rn, (const int*)rf, keys);
        EOE_CHECK_LAUNCH("feature_knn (tiles)");
    }
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)nq), dim3(64), 0, st, (const unsigned long long*)keys, nq, nr, k, chunks,
                       (const int*)qf, (const int*)rf, idx, d2, counts);
    EOE_CHECK_LAUNCH("feature_knn (merge)");
    return 0;
}
