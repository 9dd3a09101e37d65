// CLIP's text tower in one call (clip/model.py:343-356 encode_text): the host side only enqueues kernels on the caller's stream; no
// host synchronisation, no allocation.  The per-layer chain is the one of eoe_vit_block_fwd (vit.cpp) with the causal attention kernel
// and without the activations a backward pass would need.
#include "common.h"

#define TRY(expr)                   \
    do {                            \
        int rc__ = (expr);          \
        if (rc__ != 0) return rc__; \
    } while (0)

int eoe_clip_ln_rows(const float* x, const float* gamma, const float* beta, void* y, int rows, int D, float eps, int dtype, void* stream);  // clip_text.hip

namespace {

eoe_gemm_args gemm(const eoe_clip_text_fwd_args* a, const void* A, const void* B, void* C, const float* bias, int M, int N, int K) {
    eoe_gemm_args g = {};
    g.A = A; g.B = B; g.C = C; g.bias = bias;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N;
    g.dtype = a->dtype; g.epilogue = EOE_EPI_NONE; g.alpha = 1.0f;
    g.sk_workspace = a->nt_sk_workspace; g.sk_workspace_bytes = a->nt_sk_workspace ? a->nt_sk_workspace_bytes : 0;
    return g;
}

// LayerNorm of the residual stream into the 16-bit GEMM operand: the vision tower's kernel where it takes the width, else the row kernel
int layernorm(const eoe_clip_text_fwd_args* a, const float* x, const float* g, const float* b, int M, void* stream) {
    if (a->D % 256 == 0 && a->D <= 1024) return eoe_layernorm_fwd(x, a->D, g, b, a->xn, a->stats, M, a->D, a->eps, a->dtype, 0, stream);
    return eoe_clip_ln_rows(x, g, b, a->xn, M, a->D, a->eps, a->dtype, stream);
}

int check(const eoe_clip_text_fwd_args* a) {
    if (!a) return eoe_set_error(EOE_ERR_ARG, "clip_text_fwd: null args");
    if (a->n <= 0 || a->L < 1 || a->L > 128 || a->heads <= 0 || a->D != 64 * a->heads || a->layers < 0 || a->vocab <= 0 || a->embed_dim <= 0)
        return eoe_set_error(EOE_ERR_ARG, "clip_text_fwd: unsupported shape n=%d L=%d D=%d heads=%d layers=%d vocab=%d embed_dim=%d "
                             "(need D = 64*heads, 1 <= L <= 128)", a->n, a->L, a->D, a->heads, a->layers, a->vocab, a->embed_dim);
    if (a->dtype != EOE_F16 && a->dtype != EOE_BF16) return eoe_set_error(EOE_ERR_ARG, "clip_text_fwd: bad dtype %d", a->dtype);
    if (!a->tokens || !a->token_embedding || !a->positional_embedding || !a->lnf_g || !a->lnf_b || !a->proj_t || !a->x0 || !a->x1 ||
        !a->xn || !a->qkv || !a->att || !a->hact || !a->stats || !a->eot16 || !a->out)
        return eoe_set_error(EOE_ERR_ARG, "clip_text_fwd: null pointer in arguments");
    if (a->layers > 0 && (!a->ln1_g || !a->ln1_b || !a->ln2_g || !a->ln2_b || !a->b_in || !a->b_out || !a->b_fc || !a->b_proj || !a->w_in ||
                          !a->w_out || !a->w_fc || !a->w_proj))
        return eoe_set_error(EOE_ERR_ARG, "clip_text_fwd: null per-layer array");
    for (int i = 0; i < a->layers; ++i)
        if (!a->ln1_g[i] || !a->ln1_b[i] || !a->ln2_g[i] || !a->ln2_b[i] || !a->b_in[i] || !a->b_out[i] || !a->b_fc[i] || !a->b_proj[i] ||
            !a->w_in[i] || !a->w_out[i] || !a->w_fc[i] || !a->w_proj[i])
            return eoe_set_error(EOE_ERR_ARG, "clip_text_fwd: null parameter pointer in layer %d", i);
    return 0;
}

}  // namespace

extern "C" int eoe_clip_text_fwd(const eoe_clip_text_fwd_args* a, void* stream) {
    TRY(check(a));
    const int M = a->n * a->L, D = a->D, H = 4 * a->D, dt = a->dtype;
    // x = token_embedding(text) + positional_embedding                                                      (model.py:345-347)
    TRY(eoe_clip_token_embed(a->tokens, a->tok_i64, a->token_embedding, a->positional_embedding, a->x0, a->n, a->L, D, a->vocab, stream));
    for (int i = 0; i < a->layers; ++i) {
        // x1 = x0 + out_proj(attn(ln_1(x0), causal))                                                         (model.py:180-187)
        TRY(layernorm(a, a->x0, a->ln1_g[i], a->ln1_b[i], M, stream));
        eoe_gemm_args g = gemm(a, a->xn, a->w_in[i], a->qkv, a->b_in[i], M, 3 * D, D);
        TRY(eoe_gemm_nt(&g, stream));
        TRY(eoe_attn_causal_fwd(a->qkv, a->att, a->n, a->L, a->heads, dt, stream));
        g = gemm(a, a->att, a->w_out[i], a->x1, a->b_out[i], M, D, D);
        g.epilogue = EOE_EPI_RESIDUAL; g.aux = a->x0; g.ldaux = D; g.out_f32 = 1;
        TRY(eoe_gemm_nt(&g, stream));
        // x0 = x1 + c_proj(quick_gelu(c_fc(ln_2(x1))))
        TRY(layernorm(a, a->x1, a->ln2_g[i], a->ln2_b[i], M, stream));
        g = gemm(a, a->xn, a->w_fc[i], a->hact, a->b_fc[i], M, H, D);
        g.epilogue = EOE_EPI_GELU;
        TRY(eoe_gemm_nt(&g, stream));
        g = gemm(a, a->hact, a->w_proj[i], a->x0, a->b_proj[i], M, D, H);
        g.epilogue = EOE_EPI_RESIDUAL; g.aux = a->x1; g.ldaux = D; g.out_f32 = 1;
        TRY(eoe_gemm_nt(&g, stream));
    }
    // ln_final of the EOT rows, then @ text_projection                                                      (model.py:349-356)
    TRY(eoe_clip_eot_ln(a->x0, a->tokens, a->tok_i64, a->lnf_g, a->lnf_b, a->eot16, a->n, a->L, D, a->eps, dt, stream));
    eoe_gemm_args g = gemm(a, a->eot16, a->proj_t, a->out, nullptr, a->n, a->embed_dim, D);
    g.out_f32 = 1;
    return eoe_gemm_nt(&g, stream);
}
