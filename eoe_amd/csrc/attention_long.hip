// Multi-head self-attention for LONG sequences (64 < L <= EOE_ATTN_LONG_MAX_L tokens, head dim 64; ViT-B/16 at 224^2: L = 197, ViT-B/32
// at 384^2: L = 145, ViT-B/16 at 384^2: L = 577), no mask, forward and backward.  attention.hip holds one whole (image, head) in one
// wavefront's registers and stops at 64 tokens; here the sequence is cut into blocks of 64 queries x 64 keys and registers and LDS do not
// depend on L.  The products, the operand layouts and the transposing LDS reads are the fragment layer of attn_frag.h
// (v_mfma_f32_16x16x32_{f16,bf16}, scores computed TRANSPOSED so that the probabilities are already the B operand of the next product,
// ds_read_b64_tr_b16 for the operand that is summed over its rows); a workgroup is four wavefronts and wave w owns rows 16 w .. 16 w + 15 of its 64-row block, as
// in attn_bwd4_kernel.
//
// Forward, one workgroup per (image, head, 64-query block): for every 64-key block kb, in order, the K and V slabs go through two LDS
// images; S^T = K Q^T (key on the accumulator row, query on the lane), online softmax against the running maximum m of the query,
//   m' = max(m, max_key s),  alpha = exp(m - m'),  e = exp(s - m'),  l = l alpha + sum_key e,  O^T = O^T alpha + V^T e16,
// and out = O^T / l at the end.  Keys >= L get -inf (every block holds a key < L, so m' is finite and their e is exactly 0); K, V and Q
// rows >= L are read as zeros through a bounds-checked buffer resource, output rows >= L are not stored.
//
// Backward, one workgroup per (image, head), nothing saved by the forward.  The row statistics are recomputed: the backward needs a pass
// over the whole key range per query anyway before the first dS can be formed (delta = sum_key P dP, taken from fp32 values as in
// attention.hip, not from the rounded output), and that pass yields the maximum and the sum with the same S^T it computes for delta.
// What a saved log-sum-exp would spare is the running-maximum bookkeeping of that pass only, against one more saved tensor per layer, a
// store in the forward-only (frozen, scoring) path and a new field in the block argument structs.
//   phase A, per 64-query block (lane = query): pass 1 over the key blocks: S^T, dP^T = V dO^T, online (m, l, a = sum_key e dP) ->
//     lse = m + log l, delta = a / l, both kept in LDS for phase B ([L] fp32 each); pass 2 over the key blocks: S^T, dP^T again,
//     P = exp(s - lse), dS^T = P (dP^T - delta) / 8, dQ^T += K^T dS16^T in fp32 across the key blocks.
//   phase B, per 64-key block (lane = key, operands swapped): over the query blocks S = Q K^T, dP = dO V^T, P = exp(s - lse[q]),
//     dS = P (dP - delta[q]) / 8, dV^T += dO^T P16, dK^T += Q^T dS16 in fp32 across the query blocks.
// Every output element is written by exactly one lane after a loop in a fixed order: no atomics, two runs give the same bits.
//
// ROUNDING POINTS (tests/attention_long_util.py writes its rounding model from this list).  Scores, the softmax statistics (m, l, lse,
// delta), P, dP and dS are fp32 and every product accumulates in fp32.  Rounded to the 16-bit type are
//   forward   e = exp(s - running maximum), UNNORMALISED, before V^T e (the row sum l adds the unrounded e); out = O / l at the store;
//   backward  P = exp(s - lse), normalised, before dO^T P (dV);  dS, the factor 1/8 included, before K^T dS^T (dQ) and Q^T dS (dK);
//             dQ, dK, dV at the store.
// dbias (the in-projection bias gradient) keeps attn_bwd4_kernel's form: start + column sums, the Q third from the unrounded fp32 dQ, the
// V third the column sums of dO (a softmax row sums to one), the K third exact zeros (a softmax-backward row sums to zero: start keeps
// its bits); per-(image, head) partial rows in bias_scratch, then the fixed-order finish kernel.
#include "attn_frag.h"

namespace {

using namespace attn_frag;       // the LDS image (ROWB, TILEB, rswz), the fragments, the reductions, store_row16
constexpr int LPAD = (EOE_ATTN_LONG_MAX_L + 63) / 64 * 64;

// Two 64-row slabs (rows 64 blk .. 64 blk + 63 of two operands) on their way into two LDS images: wave w moves rows 16 w .. 16 w + 15,
// a lane 16 bytes of two rows per operand.  load() only issues the reads; store() waits for every wave to be done with the images' old
// content, writes, and waits until the new content is complete.
struct Slabs {
    u32x4 a[2], b[2];
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t ra, unsigned pitcha, unsigned cba, __amdgpu_buffer_rsrc_t rb, unsigned pitchb,
                                         unsigned cbb, int blk, int L, int w, int lane) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int row = 64 * blk + 16 * w + it * 8 + (lane >> 3);
            const unsigned cb = (unsigned)(lane & 7) * 16u;
            a[it] = bload16(ra, row, L, pitcha, cba + cb);
            b[it] = bload16(rb, row, L, pitchb, cbb + cb);
        }
    }
    __device__ __forceinline__ void store(char* ia, char* ib, int w, int lane) const {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int o = (16 * w + it * 8 + (lane >> 3)) * ROWB + (((lane & 7) * 16) ^ rswz(it * 8 + (lane >> 3)));
            *(u32x4*)(ia + o) = a[it];
            *(u32x4*)(ib + o) = b[it];
        }
        __syncthreads();
    }
};

// ------------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int L, int heads, int nqb, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2 * TILEB];
    char* ks_ = smem;
    char* vs = smem + TILEB;
    const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // the query blocks of one (image, head) are neighbours in the grid: they share its K and V in the L2
    const int qb = (int)(blockIdx.x % (unsigned)nqb), ih = (int)(blockIdx.x / (unsigned)nqb);
    const int img = ih / heads, h = ih % heads;
    const int D = heads * 64, ld = 3 * D;
    const unsigned pitchb = (unsigned)ld * 2u, kcb = (unsigned)D * 2u, vcb = (unsigned)D * 4u;
    const T* base = qkv + (size_t)img * L * ld + h * 64;
    // one resource over this (image, head)'s Q | K | V slices: rows of 3 D elements, the last one ending behind V's 64 columns
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(base, ((unsigned)(L - 1) * (unsigned)ld + 2u * D + 64u) * 2u);
    const int nkb = (L + 63) >> 6;
    const int mine = 64 * qb + 16 * w + lr;                  // this lane's query

    V8<T> qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = rowfrag<T>(rq, pitchb, 0u, L, mine, ks, lane);
    f32x4 o[4];              // O^T: tile td, register r of lane (lr, lg) = d 16 lg + 4 td + r of query `mine`
#pragma unroll
    for (int td = 0; td < 4; ++td) o[td] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float mrun = -INFINITY, lrun = 0.f;                      // lrun: this lane's share of the row sum (alpha is the same in the 4 lanes of a query)

    Slabs sl;
    sl.load(rq, pitchb, kcb, rq, pitchb, vcb, 0, L, w, lane);
    for (int kb = 0; kb < nkb; ++kb) {
        sl.store(ks_, vs, w, lane);
        if (kb + 1 < nkb) sl.load(rq, pitchb, kcb, rq, pitchb, vcb, kb + 1, L, w, lane);      // in flight under this block's products
        f32x4 s[4];
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) s[tk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk) s[tk] = T16<T>::mfma16(lfrag<T>(ks_, tk, ks, lane), qf[ks], s[tk]);
        float m = -INFINITY;
#pragma unroll
        for (int tk = 0; tk < 4; ++tk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 64 * kb + 16 * tk + 4 * lg + r;
                const float v = (key < L) ? s[tk][r] * scale : -INFINITY;
                s[tk][r] = v;
                m = fmaxf(m, v);
            }
        const float mnew = fmaxf(mrun, group_max(m));        // finite: key 64 kb < L
        const float alpha = __expf(mrun - mnew);
        float sum = 0.f;
#pragma unroll
        for (int tk = 0; tk < 4; ++tk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(s[tk][r] - mnew);
                s[tk][r] = e;
                sum += e;
            }
        lrun = lrun * alpha + sum;
        mrun = mnew;
#pragma unroll
        for (int td = 0; td < 4; ++td) {
            o[td] *= alpha;
#pragma unroll
            for (int st = 0; st < 2; ++st)
                o[td] = T16<T>::mfma16(tfrag_il<T>(vs, td, st, lane), acc_as_operand<T>(s[2 * st], s[2 * st + 1]), o[td]);
        }
    }
    const float inv = 1.0f / group_sum(lrun);
    u32x2 pk[4];
#pragma unroll
    for (int td = 0; td < 4; ++td) pk[td] = pack4<T>(o[td][0] * inv, o[td][1] * inv, o[td][2] * inv, o[td][3] * inv);
    if (mine < L) store_row16(out + ((size_t)img * L + mine) * D + h * 64 + 16 * lg, pk);
}

// ------------------------------------------------------------------------------------------------ backward
template <typename T>
__global__ __launch_bounds__(256) void attn_long_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ dout, T* __restrict__ dqkv,
                                                            float* __restrict__ bias_part, int L, int heads, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[2 * TILEB + 2 * LPAD * 4 + 4 * 192 * 4];
    char* ia = smem;                                          // phase A: K   phase B: Q
    char* ib = smem + TILEB;                                  // phase A: V   phase B: dO
    float* lse_s = (float*)(smem + 2 * TILEB);
    float* dlt_s = lse_s + LPAD;
    float* red = dlt_s + LPAD;                                // [4 waves][dQ | dK | dV column sums, 64 each]

    const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int img = blockIdx.x / heads, h = blockIdx.x % heads;
    const int D = heads * 64, ld = 3 * D;
    const T* qp = qkv + (size_t)img * L * ld + h * 64;
    const T* dop = dout + (size_t)img * L * D + h * 64;
    T* dqp = dqkv + (size_t)img * L * ld + h * 64;
    const unsigned pitchb = (unsigned)ld * 2u, pitchd = (unsigned)D * 2u, kcb = (unsigned)D * 2u, vcb = (unsigned)D * 4u;
    const __amdgpu_buffer_rsrc_t rq = make_rsrc(qp, ((unsigned)(L - 1) * (unsigned)ld + 2u * D + 64u) * 2u);
    const __amdgpu_buffer_rsrc_t rdo = make_rsrc(dop, ((unsigned)(L - 1) * (unsigned)D + 64u) * 2u);
    const int nb = (L + 63) >> 6;
    // this (image, head)'s column sums of dQ | dK | dV -> partial row `img` in the blocked layout (attention.hip)
    const int n_img = gridDim.x / heads;
    float* bpart = bias_part ? bias_part + ((size_t)h * n_img + img) * 64 : nullptr;
    const size_t bseg = (size_t)heads * n_img * 64;
    float* myred = red + w * 192;
    Slabs sl;

    // ---- phase A: lane = query.  S^T = K Q^T, dP^T = V dO^T
    f32x4 csq[4];                                             // column sums of this wave's dQ rows, over the query blocks
#pragma unroll
    for (int td = 0; td < 4; ++td) csq[td] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < nb; ++qb) {
        const int mine = 64 * qb + 16 * w + lr;
        V8<T> qf[2], df[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[ks] = rowfrag<T>(rq, pitchb, 0u, L, mine, ks, lane);
            df[ks] = rowfrag<T>(rdo, pitchd, 0u, L, mine, ks, lane);
        }
        // pass 1: the row statistics.  m: running maximum; l, a: this lane's shares of sum e and sum e dP (alpha is the same in a query's 4 lanes)
        float mrun = -INFINITY, lrun = 0.f, arun = 0.f;
        for (int kb = 0; kb < nb; ++kb) {
            sl.load(rq, pitchb, kcb, rq, pitchb, vcb, kb, L, w, lane);
            sl.store(ia, ib, w, lane);
            f32x4 s[4], dp[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                dp[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int tk = 0; tk < 4; ++tk) {
                    s[tk] = T16<T>::mfma16(lfrag<T>(ia, tk, ks, lane), qf[ks], s[tk]);
                    dp[tk] = T16<T>::mfma16(lfrag<T>(ib, tk, ks, lane), df[ks], dp[tk]);
                }
            float m = -INFINITY;
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 64 * kb + 16 * tk + 4 * lg + r;
                    const float v = (key < L) ? s[tk][r] * scale : -INFINITY;
                    s[tk][r] = v;
                    m = fmaxf(m, v);
                }
            const float mnew = fmaxf(mrun, group_max(m));
            const float alpha = __expf(mrun - mnew);
            float sum = 0.f, sdp = 0.f;
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __expf(s[tk][r] - mnew);          // keys >= L: 0, and their dP is 0 (V rows read as zeros)
                    sum += e;
                    sdp += e * dp[tk][r];
                }
            lrun = lrun * alpha + sum;
            arun = arun * alpha + sdp;
            mrun = mnew;
        }
        const float lsum = group_sum(lrun);
        const float lse = mrun + __logf(lsum), dl = group_sum(arun) / lsum;
        // rows >= L of the last block: P = exp(s - inf) = 0 and dS = 0 in phase B
        if (lg == 0) {
            lse_s[mine] = mine < L ? lse : INFINITY;
            dlt_s[mine] = mine < L ? dl : 0.f;
        }
        // pass 2: dS^T = P^T (dP^T - delta) * scale;  dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q]
        f32x4 o[4];
#pragma unroll
        for (int td = 0; td < 4; ++td) o[td] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nb; ++kb) {
            sl.load(rq, pitchb, kcb, rq, pitchb, vcb, kb, L, w, lane);
            sl.store(ia, ib, w, lane);
            f32x4 s[4], dp[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                dp[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int tk = 0; tk < 4; ++tk) {
                    s[tk] = T16<T>::mfma16(lfrag<T>(ia, tk, ks, lane), qf[ks], s[tk]);
                    dp[tk] = T16<T>::mfma16(lfrag<T>(ib, tk, ks, lane), df[ks], dp[tk]);
                }
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 64 * kb + 16 * tk + 4 * lg + r;
                    const float p = (key < L) ? __expf(s[tk][r] * scale - lse) : 0.f;
                    dp[tk][r] = p * (dp[tk][r] - dl) * scale;
                }
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int st = 0; st < 2; ++st)
                    o[td] = T16<T>::mfma16(tfrag_il<T>(ia, td, st, lane), acc_as_operand<T>(dp[2 * st], dp[2 * st + 1]), o[td]);
        }
        // tile td, register r of lane (lr, lg) = d 16 lg + 4 td + r: the lane's four tiles are 16 consecutive d of its query's row
        u32x2 pk[4];
#pragma unroll
        for (int td = 0; td < 4; ++td) {
            pk[td] = pack4<T>(o[td][0], o[td][1], o[td][2], o[td][3]);
            csq[td] += slab_sum(o[td], mine < L);
        }
        if (mine < L) store_row16(dqp + (size_t)mine * ld + 16 * lg, pk);
    }

    // ---- phase B: lane = key (operands swapped).  S = Q K^T, dP = dO V^T; rows (registers) = queries
    float cdo[8];                                             // this lane's share of the column sums of dO (8 columns from 8 (lane & 7))
#pragma unroll
    for (int j = 0; j < 8; ++j) cdo[j] = 0.f;
    for (int kb = 0; kb < nb; ++kb) {
        const int mine = 64 * kb + 16 * w + lr;
        V8<T> kf[2], vf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[ks] = rowfrag<T>(rq, pitchb, kcb, L, mine, ks, lane);
            vf[ks] = rowfrag<T>(rq, pitchb, vcb, L, mine, ks, lane);
        }
        f32x4 ov[4], ok[4];
#pragma unroll
        for (int td = 0; td < 4; ++td) {
            ov[td] = (f32x4){0.f, 0.f, 0.f, 0.f};
            ok[td] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        for (int qb = 0; qb < nb; ++qb) {
            sl.load(rq, pitchb, 0u, rdo, pitchd, 0u, qb, L, w, lane);
            if (kb == 0) {
                // every dO slab passes through here once per key block: the first time round its rows (zeros behind L) are summed
                float a0[8], a1[8];
                unpack8<T>(sl.b[0], a0);
                unpack8<T>(sl.b[1], a1);
#pragma unroll
                for (int j = 0; j < 8; ++j) cdo[j] += a0[j] + a1[j];
            }
            sl.store(ia, ib, w, lane);          // (its first barrier also puts phase A's lse / delta stores in front of the reads below)
            f32x4 s[4], dp[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                dp[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) {
                    s[tq] = T16<T>::mfma16(lfrag<T>(ia, tq, ks, lane), kf[ks], s[tq]);
                    dp[tq] = T16<T>::mfma16(lfrag<T>(ib, tq, ks, lane), vf[ks], dp[tq]);
                }
            // P = exp(S*scale - lse[q]);  dS = P (dP - delta[q]) * scale
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                const f32x4 lse = *(const f32x4*)(lse_s + 64 * qb + 16 * tq + 4 * lg);
                const f32x4 dl = *(const f32x4*)(dlt_s + 64 * qb + 16 * tq + 4 * lg);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __expf(s[tq][r] * scale - lse[r]);
                    s[tq][r] = p;
                    dp[tq][r] = p * (dp[tq][r] - dl[r]) * scale;
                }
            }
            // dV^T[d][key] += sum_q dO^T[d][q] P[q][key] ;  dK^T[d][key] += sum_q Q^T[d][q] dS[q][key]
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    ov[td] = T16<T>::mfma16(tfrag_il<T>(ib, td, st, lane), acc_as_operand<T>(s[2 * st], s[2 * st + 1]), ov[td]);
                    ok[td] = T16<T>::mfma16(tfrag_il<T>(ia, td, st, lane), acc_as_operand<T>(dp[2 * st], dp[2 * st + 1]), ok[td]);
                }
        }
        // (a key >= L holds whatever exp(-lse) gives: its column is its own and is not stored)
        if (mine < L) {
            u32x2 pv[4], pk[4];
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                pv[td] = pack4<T>(ov[td][0], ov[td][1], ov[td][2], ov[td][3]);
                pk[td] = pack4<T>(ok[td][0], ok[td][1], ok[td][2], ok[td][3]);
            }
            T* dv = dqp + (size_t)mine * ld + 2 * D + 16 * lg;
            T* dk = dqp + (size_t)mine * ld + D + 16 * lg;
            store_row16(dv, pv);
            store_row16(dk, pk);
        }
    }
    if (bpart) {
        // per-wave partials, summed in wave order: dQ from the accumulators, dK exact zeros, dV the column sums of dO (file header)
        if (lr == 0) {
#pragma unroll
            for (int td = 0; td < 4; ++td) *(f32x4*)(myred + 16 * lg + 4 * td) = csq[td];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = cdo[j];
            v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
            cdo[j] = v;
        }
        if (lane < 8) {
            *(f32x4*)(myred + 128 + 8 * lane) = (f32x4){cdo[0], cdo[1], cdo[2], cdo[3]};
            *(f32x4*)(myred + 128 + 8 * lane + 4) = (f32x4){cdo[4], cdo[5], cdo[6], cdo[7]};
        } else if (lane < 24) {
            *(f32x4*)(myred + 64 + 4 * (lane - 8)) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < 192) bpart[(size_t)(t >> 6) * bseg + (t & 63)] = (red[t] + red[192 + t]) + (red[384 + t] + red[576 + t]);
    }
}

int check_long(const char* who, int n, int L, int heads, int dtype) {
    EOE_CHECK_ARG(n > 0 && heads > 0, "%s: bad args", who);
    EOE_CHECK_ARG(L > 64 && L <= EOE_ATTN_LONG_MAX_L, "%s: sequence length %d not in [65, %d]", who, L, EOE_ATTN_LONG_MAX_L);
    EOE_CHECK_ARG(dtype == EOE_F16 || dtype == EOE_BF16, "%s: bad dtype %d", who, dtype);
    EOE_CHECK_ARG((double)n * heads * ((L + 63) / 64) < 2147483647.0, "%s: too many workgroups", who);
    return 0;
}

}  // namespace

extern "C" int eoe_attn_long_fwd(const void* qkv, void* out, int n, int L, int heads, int dtype, void* stream) {
    EOE_CHECK_ARG(qkv && out, "attn_long_fwd: bad args");
    EOE_TRY(check_long("attn_long_fwd", n, L, heads, dtype));
    const float scale = 0.125f;   // 1/sqrt(64)
    const int nqb = (L + 63) / 64;
    ProfScope ps("attn_long_fwd", 4.0 * n * heads * (double)L * L * 64, 2.0 * (double)n * L * heads * 64 * 4, stream);
    if (dtype == EOE_F16)
        hipLaunchKernelGGL((attn_long_fwd_kernel<f16_t>), dim3(n * heads * nqb), dim3(256), 0, (hipStream_t)stream,
                           (const f16_t*)qkv, (f16_t*)out, L, heads, nqb, scale);
    else
        hipLaunchKernelGGL((attn_long_fwd_kernel<bf16_t>), dim3(n * heads * nqb), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)qkv, (bf16_t*)out, L, heads, nqb, scale);
    EOE_CHECK_LAUNCH("attn_long_fwd");
    return 0;
}

extern "C" int eoe_attn_long_bwd(const void* qkv, const void* dout, void* dqkv, float* dbias, float* bias_scratch, int n, int L,
                                 int heads, int dtype, void* stream) {
    EOE_CHECK_ARG(qkv && dout && dqkv, "attn_long_bwd: bad args");
    EOE_CHECK_ARG((dbias == nullptr) == (bias_scratch == nullptr), "attn_long_bwd: dbias and bias_scratch go together");
    EOE_TRY(check_long("attn_long_bwd", n, L, heads, dtype));
    const float scale = 0.125f;
    // nine products per (query block, key block): S^T and dP^T twice and dQ in phase A, S, dP, dV and dK in phase B
    ProfScope ps("attn_long_bwd", 18.0 * n * heads * (double)L * L * 64, 2.0 * (double)n * L * heads * 64 * 7, stream);
    if (dtype == EOE_F16)
        hipLaunchKernelGGL((attn_long_bwd_kernel<f16_t>), dim3(n * heads), dim3(256), 0, (hipStream_t)stream,
                           (const f16_t*)qkv, (const f16_t*)dout, (f16_t*)dqkv, bias_scratch, L, heads, scale);
    else
        hipLaunchKernelGGL((attn_long_bwd_kernel<bf16_t>), dim3(n * heads), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)qkv, (const bf16_t*)dout, (bf16_t*)dqkv, bias_scratch, L, heads, scale);
    EOE_CHECK_LAUNCH("attn_long_bwd");
    if (dbias) EOE_TRY(eoe_finish_reduce(bias_scratch, n, 3 * heads * 64, 3 * heads * 64, dbias, nullptr, nullptr, 1, stream));
    return 0;
}
