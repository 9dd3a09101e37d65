// CLIP's text tower (clip/model.py:343-356 encode_text): the kernels the vision tower does not have.
//   * causal multi-head attention (the mask of CLIP.build_attention_mask, model.py:284-290) over up to 128 tokens, head dim 64;
//   * the token embedding gather + positional embedding (model.py:345-347) into the fp32 residual stream;
//   * the EOT head: first-occurrence argmax of the token ids (text.argmax(dim=-1), model.py:354) and ln_final of that row only;
//   * a LayerNorm over rows of any width D % 64 == 0 (the driver calls eoe_layernorm_fwd at D % 256 == 0 and this one elsewhere).
// The layer chain itself (LayerNorm, GEMMs with their epilogues) is eoe_clip_text_fwd in clip_text_driver.cpp.
//
// Attention: one wavefront per (sequence, head, 64-query block).  The products follow attn_fwd_kernel (attention.hip) on the fragment
// layer of attn_frag.h (LDS image, bounds-checked loads, operand fragments, lane-group reductions): scores are computed TRANSPOSED (S^T = K Q^T, key on the accumulator row, query on the lane), so the probabilities are already the B operand of
// O^T = V^T P^T, with V read back through ds_read_b64_tr_b16 from an LDS image.  A query block visits the key blocks kb <= qb only (the
// blocks above the diagonal are skipped) with an online softmax across them; keys j > i inside the diagonal block get -inf, so they
// add exact zeros to the row sum and to the output.  Q, K and V rows >= L are read through a bounds-checked buffer resource as zeros,
// and output rows >= L are not stored.
#include "attn_frag.h"

namespace {

using namespace attn_frag;       // the LDS image (ROWB, TILEB, rswz), the fragments, the reductions, qkv_rsrc, store_row16

template <typename T>
__global__ __launch_bounds__(64) void attn_causal_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int L, int heads, int nqb,
                                                             float scale) {
    __shared__ __attribute__((aligned(16))) char vs[2][TILEB];
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    // the blocks of the last query block (the most key blocks) first
    const int qb = nqb - 1 - (int)(blockIdx.x % (unsigned)nqb);
    const int sh = (int)(blockIdx.x / (unsigned)nqb);
    const int seq = sh / heads, h = sh % heads;
    const int D = heads * 64, ld = 3 * D;
    const unsigned pitchb = (unsigned)ld * 2u, kcb = (unsigned)D * 2u, vcb = (unsigned)D * 4u;
    const T* base = qkv + (size_t)seq * L * ld + h * 64;

    const int Lq = min(64, L - qb * 64);
    const __amdgpu_buffer_rsrc_t rq = qkv_rsrc(base + (size_t)qb * 64 * ld, Lq, ld, D);
    V8<T> qf[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < 4; ++t) qf[ks][t] = bfrag<T>(rq, pitchb, 0u, Lq, t, ks, lane);

    f32x4 o[4][4];           // O^T: [d-tile td][query tile tq], d on the accumulator row, query on the lane
#pragma unroll
    for (int td = 0; td < 4; ++td)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) o[td][tq] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float mrun[4], lrun[4];
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) mrun[tq] = -INFINITY, lrun[tq] = 0.f;

    for (int kb = 0; kb <= qb; ++kb) {
        const int Lk = min(64, L - kb * 64);
        const __amdgpu_buffer_rsrc_t rk = qkv_rsrc(base + (size_t)kb * 64 * ld, Lk, ld, D);
        char* vimg = vs[kb];
        u32x4 vv[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) vv[it] = bload16(rk, it * 8 + (lane >> 3), Lk, pitchb, vcb + (unsigned)(lane & 7) * 16u);
        V8<T> kf[2][4];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int t = 0; t < 4; ++t) kf[ks][t] = bfrag<T>(rk, pitchb, kcb, Lk, t, ks, lane);
#pragma unroll
        for (int it = 0; it < 8; ++it) *(u32x4*)(vimg + (it * 8 + (lane >> 3)) * ROWB + (((lane & 7) * 16) ^ rswz(it * 8 + (lane >> 3)))) = vv[it];

        f32x4 s[4][4];       // S^T: [key tile tk][query tile tq]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) s[tk][tq] = T16<T>::mfma16(kf[ks][tk], qf[ks][tq], s[tk][tq]);

        // mask + online softmax.  Every query of block qb has a valid key in every block kb <= qb (key kb*64 <= query, kb*64 < L), so the
        // running maximum is finite after the first block and exp(-inf - m) = 0 exactly for the masked keys.
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
            const int query = qb * 64 + 16 * tq + lr;
            float m = -INFINITY;
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kb * 64 + 16 * tk + 4 * lg + r;
                    const float v = (key <= query && key < L) ? s[tk][tq][r] * scale : -INFINITY;
                    s[tk][tq][r] = v;
                    m = fmaxf(m, v);
                }
            const float mnew = fmaxf(mrun[tq], group_max(m));
            const float alpha = __expf(mrun[tq] - mnew);
            float sum = 0.f;
#pragma unroll
            for (int tk = 0; tk < 4; ++tk)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __expf(s[tk][tq][r] - mnew);
                    s[tk][tq][r] = e;
                    sum += e;
                }
            lrun[tq] = lrun[tq] * alpha + group_sum(sum);
            mrun[tq] = mnew;
#pragma unroll
            for (int td = 0; td < 4; ++td) o[td][tq] *= alpha;
        }

        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int td = 0; td < 4; ++td)
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const V8<T> vf = tfrag_il<T>(vimg, td, st, lane);
#pragma unroll
                for (int tq = 0; tq < 4; ++tq)
                    o[td][tq] = T16<T>::mfma16(vf, acc_as_operand<T>(s[2 * st][tq], s[2 * st + 1][tq]), o[td][tq]);
            }
    }

    // lane (lr, lg) of tile (td, tq) holds d = 16 lg + 4 td + 0..3 of query 16 tq + lr: two 16-byte stores per query tile
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) {
        const int query = 16 * tq + lr;
        const float inv = 1.0f / lrun[tq];
        u32x2 pk[4];
#pragma unroll
        for (int td = 0; td < 4; ++td) pk[td] = pack4<T>(o[td][tq][0] * inv, o[td][tq][1] * inv, o[td][tq][2] * inv, o[td][tq][3] * inv);
        if (query < Lq) store_row16(out + ((size_t)seq * L + qb * 64 + query) * D + h * 64 + 16 * lg, pk);
    }
}

// ------------------------------------------------------------------------------------------------ token embedding
// out[s*L + t, :] = emb[tok[s, t], :] + pos[t, :]; one thread per 4 columns.  An id outside [0, vocab) is clamped (the host wrapper
// rejects such ids before the launch; the clamp only keeps the gather inside the table).
template <typename I>
__global__ __launch_bounds__(256) void token_embed_kernel(const I* __restrict__ tok, const float* __restrict__ emb, const float* __restrict__ pos,
                                                          float* __restrict__ out, int M, int L, int D, int vocab) {
    const int q4 = D >> 2;
    const size_t total = (size_t)M * q4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / q4), c = (int)(i % q4) * 4, t = row % L;
        long long id = (long long)tok[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const f32x4 e = *(const f32x4*)(emb + (size_t)id * D + c);
        const f32x4 p = *(const f32x4*)(pos + (size_t)t * D + c);
        *(f32x4*)(out + (size_t)row * D + c) = e + p;
    }
}

// ------------------------------------------------------------------------------------------------ LayerNorm of single rows
// y[r, :] (16-bit) = LayerNorm(x[src(r), :]) with fp32 statistics, biased variance (model.py:153-159); one wavefront per row, any
// D % 4 == 0.  src(r) = r (plain rows), or, with `tok`, row r*L + argmax_t tok[r, t] (the EOT head: the first position of the largest id).
template <typename T, typename I>
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* __restrict__ x, const I* __restrict__ tok, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, T* __restrict__ y, int rows, int L, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    size_t src = (size_t)r;
    if (tok) {
        long long best = (long long)(-0x7fffffffffffffffLL - 1);
        int at = 0;
        for (int t = lane; t < L; t += 64) {
            const long long v = (long long)tok[(size_t)r * L + t];
            if (v > best) best = v, at = t;            // strictly greater: the first of equal ids within the lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long ob = __shfl_xor(best, o, 64);
            const int oat = __shfl_xor(at, o, 64);
            if (ob > best || (ob == best && oat < at)) best = ob, at = oat;
        }
        src = (size_t)r * L + at;
    }
    const float* xr = x + src * D;
    float s = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        s += v[0] + v[1] + v[2] + v[3];
    }
    const float mean = wave_sum(s) / D;
    float q = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) q += (v[k] - mean) * (v[k] - mean);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / D + eps);
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c), g = *(const f32x4*)(gamma + c), b = *(const f32x4*)(beta + c);
        *(u32x2*)(y + (size_t)r * D + c) = pack4<T>((v[0] - mean) * rstd * g[0] + b[0], (v[1] - mean) * rstd * g[1] + b[1],
                                                    (v[2] - mean) * rstd * g[2] + b[2], (v[3] - mean) * rstd * g[3] + b[3]);
    }
}

template <typename T>
int launch_ln_rows(const float* x, const void* tok, int tok_i64, const float* gamma, const float* beta, void* y, int rows, int L, int D,
                   float eps, hipStream_t s) {
    const dim3 grid(cdiv(rows, 4)), block(256);
    if (!tok)
        hipLaunchKernelGGL((ln_rows_kernel<T, int32_t>), grid, block, 0, s, x, nullptr, gamma, beta, (T*)y, rows, L, D, eps);
    else if (tok_i64)
        hipLaunchKernelGGL((ln_rows_kernel<T, int64_t>), grid, block, 0, s, x, (const int64_t*)tok, gamma, beta, (T*)y, rows, L, D, eps);
    else
        hipLaunchKernelGGL((ln_rows_kernel<T, int32_t>), grid, block, 0, s, x, (const int32_t*)tok, gamma, beta, (T*)y, rows, L, D, eps);
    return 0;
}

}  // namespace

extern "C" int eoe_attn_causal_fwd(const void* qkv, void* out, int n, int L, int heads, int dtype, void* stream) {
    EOE_CHECK_ARG(qkv && out, "attn_causal_fwd: null pointer");
    EOE_CHECK_ARG(n > 0 && heads > 0 && L >= 1 && L <= 128, "attn_causal_fwd: unsupported shape n=%d L=%d heads=%d (1 <= L <= 128)", n, L, heads);
    EOE_CHECK_ARG(dtype == EOE_F16 || dtype == EOE_BF16, "attn_causal_fwd: bad dtype %d", dtype);
    EOE_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "attn_causal_fwd: qkv / out must be 16-byte aligned");
    const int nqb = cdiv(L, 64);
    const double keys = 0.5 * L * (L + 1);
    ProfScope ps("attn_causal_fwd", 4.0 * n * heads * 64 * keys, 2.0 * n * L * heads * 64 * 4, stream);
    const dim3 grid((unsigned)(n * heads * nqb)), block(64);
    if (dtype == EOE_F16)
        hipLaunchKernelGGL(attn_causal_fwd_kernel<f16_t>, grid, block, 0, (hipStream_t)stream, (const f16_t*)qkv, (f16_t*)out, L, heads, nqb, 0.125f);
    else
        hipLaunchKernelGGL(attn_causal_fwd_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)out, L, heads, nqb, 0.125f);
    EOE_CHECK_LAUNCH("attn_causal_fwd");
    return 0;
}

extern "C" int eoe_clip_token_embed(const void* tok, int tok_i64, const float* token_embedding, const float* positional_embedding,
                                    float* out, int n, int L, int D, int vocab, void* stream) {
    EOE_CHECK_ARG(tok && token_embedding && positional_embedding && out, "clip_token_embed: null pointer");
    EOE_CHECK_ARG(n > 0 && L > 0 && D > 0 && D % 4 == 0 && vocab > 0, "clip_token_embed: bad shape n=%d L=%d D=%d vocab=%d", n, L, D, vocab);
    ProfScope ps("clip_token_embed", 0, 12.0 * n * L * D, stream);
    const int M = n * L;
    const size_t want = ((size_t)M * (D / 4) + 255) / 256;
    const int blocks = (int)(want < 4096 ? want : 4096);
    if (tok_i64)
        hipLaunchKernelGGL(token_embed_kernel<int64_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const int64_t*)tok, token_embedding,
                           positional_embedding, out, M, L, D, vocab);
    else
        hipLaunchKernelGGL(token_embed_kernel<int32_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const int32_t*)tok, token_embedding,
                           positional_embedding, out, M, L, D, vocab);
    EOE_CHECK_LAUNCH("clip_token_embed");
    return 0;
}

extern "C" int eoe_clip_eot_ln(const float* x, const void* tok, int tok_i64, const float* gamma, const float* beta, void* y, int n, int L,
                               int D, float eps, int dtype, void* stream) {
    EOE_CHECK_ARG(x && tok && gamma && beta && y, "clip_eot_ln: null pointer");
    EOE_CHECK_ARG(n > 0 && L > 0 && D > 0 && D % 4 == 0, "clip_eot_ln: bad shape n=%d L=%d D=%d", n, L, D);
    EOE_CHECK_ARG(dtype == EOE_F16 || dtype == EOE_BF16, "clip_eot_ln: bad dtype %d", dtype);
    ProfScope ps("clip_eot_ln", 0, 8.0 * n * L + 14.0 * n * D, stream);
    if (dtype == EOE_F16) launch_ln_rows<f16_t>(x, tok, tok_i64, gamma, beta, y, n, L, D, eps, (hipStream_t)stream);
    else launch_ln_rows<bf16_t>(x, tok, tok_i64, gamma, beta, y, n, L, D, eps, (hipStream_t)stream);
    EOE_CHECK_LAUNCH("clip_eot_ln");
    return 0;
}

// plain rows (clip_text_driver.cpp: the text tower's LayerNorm-1 / -2 where eoe_layernorm_fwd does not take the width)
int eoe_clip_ln_rows(const float* x, const float* gamma, const float* beta, void* y, int rows, int D, float eps, int dtype, void* stream) {
    EOE_CHECK_ARG(x && gamma && beta && y && rows > 0 && D > 0 && D % 4 == 0, "clip_ln_rows: bad args");
    ProfScope ps("clip_ln_rows", 0, 14.0 * rows * D, stream);
    if (dtype == EOE_F16) launch_ln_rows<f16_t>(x, nullptr, 0, gamma, beta, y, rows, 1, D, eps, (hipStream_t)stream);
    else launch_ln_rows<bf16_t>(x, nullptr, 0, gamma, beta, y, rows, 1, D, eps, (hipStream_t)stream);
    EOE_CHECK_LAUNCH("clip_ln_rows");
    return 0;
}
