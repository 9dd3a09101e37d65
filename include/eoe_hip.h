/* eoe_hip.h -- C ABI of libeoe_hip.so: the MI355X (gfx950) kernels of the outlier-exposure AD training hot path.
 *
 * The reference (liznerski/eoe) is pure Python and has no FFI; its boundary for this path is the duck-typed
 * torch.nn.Module / ADTrainer-hook interface.  Every entry point below names the
 * reference call it replaces (path:line relative to /root/reference).  Conventions:
 *   - plain pointers and sizes only; the caller (PyTorch) owns every buffer, including workspaces;
 *   - every call takes the HIP stream to launch on (`void* stream` = hipStream_t);
 *   - return 0 on success, non-zero on error; the message is in the thread-local eoe_last_error();
 *   - "16-bit" buffers hold IEEE fp16 (EOE_F16) or bfloat16 (EOE_BF16), chosen per call with `dtype`;
 *     accumulation, LayerNorm statistics, the residual stream, losses, gradients of parameters and the
 *     optimiser state are fp32;
 *   - token tensors are batch-major:  row = image * L + token  (the reference's LND permute,
 *     clip/model.py:227,229, is value-preserving).
 */
#ifndef EOE_HIP_H
#define EOE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EOE_ABI_VERSION 5

enum { EOE_OK = 0, EOE_ERR_ARG = 1, EOE_ERR_LAUNCH = 2, EOE_ERR_UNSUPPORTED = 3 };
enum { EOE_F16 = 1, EOE_BF16 = 2, EOE_F32 = 3 /* only where an entry point says so */ };

int eoe_abi_version(void);
/* sizeof of an argument struct as compiled into the library: 0 eoe_gemm_args, 1 eoe_conv_geometry, 2 eoe_adam_chunk,
 * 3 eoe_adam_scalars, 4/5 eoe_vit_block_fwd/bwd_args, 6/7 eoe_cgate(_bwd)_args, 8/9 eoe_sgate(_bwd)_args, 10 eoe_adam_tile, 11 eoe_red_table;
 * -1 otherwise */
int eoe_struct_size(int which);
const char* eoe_last_error(void);

/* ------------------------------------------------------------------------------------------------------
 * GEMM (MFMA 16x16x32, LDS-staged 128x128x64 tiles, fp32 accumulate)
 *   replaces: every nn.Linear / F.linear / conv1-as-GEMM / `x @ proj` on the path
 *   (clip/model.py:171-178,220,233-234; custom_base.py:25-26,47-48) and their autograd backward
 *   (ad_trainer.py:431).
 *   NT:  C[M,N] = A[M,K] . B[N,K]^T            (forward: B = weight;  dgrad: B = transposed weight copy)
 *   TN:  C[M,N] = A[T,M]^T . B[T,N]            (wgrad: A = dY, B = X, reduction over the T tokens)
 * ---------------------------------------------------------------------------------------------------- */
enum {
    EOE_EPI_NONE = 0,      /* C = acc (+ bias)                                                         */
    EOE_EPI_GELU = 1,      /* pre = acc + bias -> aux_out (16-bit; NULL: not kept);  C = pre * sigmoid(1.702 pre) of the ROUNDED pre */
    EOE_EPI_RESIDUAL = 2,  /* C(fp32) = acc + bias + aux(fp32 [M,N], leading dim ldaux)                */
    EOE_EPI_GELU_BWD = 3   /* C = acc * d/dpre[pre sigmoid(1.702 pre)],  pre = aux (16-bit [M,N])      */
};

/* geometry of a convolution whose patch matrix is never materialised ("implicit GEMM": the GEMM kernel fetches every
 * 16-byte piece -- 8 channels of one tap of one output pixel -- from the 16-bit NHWC activation [n, H, W, C] straight into
 * its LDS stage; taps in the zero padding arrive as zeros).  Patch row = output pixel (img, ho, wo) of the Ho x Wo grid,
 * patch column = (ky*kw + kx)*C + c  ->  element (img, ho*stride - pad + ky, wo*stride - pad + kx, c). */
typedef struct {
    int32_t n, H, W, C;           /* gathered tensor */
    int32_t kh, kw, stride, pad;
    int32_t Ho, Wo;               /* grid of patch rows */
} eoe_conv_geometry;

typedef struct {
    const void* A;      /* 16-bit */
    const void* B;      /* 16-bit */
    void* C;            /* 16-bit, or fp32 if out_f32 */
    const float* bias;  /* [N] fp32 or NULL */
    const void* aux;    /* see epilogue */
    void* aux_out;      /* see epilogue */
    float* colsum;      /* optional (NT only): colsum[n] += sum_m C[m,n] of the epilogue result -- fp32 atomics, or, with a
                         * workspace of >= EOE_NT_COLSUM_WORKSPACE_BYTES(M, N), per-wave partial rows added up by a second kernel
                         * in a fixed order (bitwise reproducible; the atomics cost +45 us on a 12800 x 3072 output) */
    int32_t M, N, K;    /* for TN, K is the reduction length T */
    int32_t lda, ldb, ldc, ldaux;   /* leading dimensions in elements */
    int32_t dtype;      /* EOE_F16 | EOE_BF16 */
    int32_t epilogue;   /* EOE_EPI_* */
    int32_t out_f32;    /* C is fp32 */
    int32_t accumulate; /* C += result (C must be fp32) */
    float alpha;        /* result scale applied to acc before bias/epilogue (1.0 = none) */
    void* workspace;    /* optional (TN): scratch for the per-split partial results of a split reduction; with
                         * workspace_bytes >= EOE_TN_WORKSPACE_BYTES the splits are summed by a second kernel instead of fp32
                         * atomics (faster, and bitwise reproducible).  With >= EOE_TN_STREAMK_WORKSPACE_BYTES(#CUs) a group
                         * whose tiles fill most but not all of the CUs once (216 of 256) runs as #CUs equal k-ranges (stream-K;
                         * the first problem's workspace is the one used) */
    int64_t workspace_bytes;
    int32_t gather;     /* 1: A is the NHWC tensor of `geo` and stands for its patch matrix (lda ignored).
                         *    NT: [M = n*Ho*Wo, K = kh*kw*C], C % 64 == 0 (one tap per 64-deep k-tile), or C in {8,16,32} with K
                         *        = kh*kw*C rounded up to a multiple of 64 (every 16-byte piece decodes its own tap); plain epilogue
                         *        (conv forward; stride-1 dgrad)
                         *    TN: [T = n*Ho*Wo, M = kh*kw*C], C % 8 == 0 (conv wgrad, transposed: C[kh*kw*C, cout])
                         * 2: A is the zero-padded NHWC4 image of eoe_stem_pack_image (geo.C = 4, geo.pad = 0, geo.H/W = Hp/Wp),
                         *    K (NT) / M (TN) = ceil(kh/2)*64 */
    eoe_conv_geometry geo;
    int32_t colstats;   /* NT only: the workspace (>= 2 * EOE_NT_COLSUM_WORKSPACE_BYTES(M, N)) receives, per 64 output rows, the column
                         * sums and sums of squares of the fp32 epilogue result: [ceil(M/64)][2][N] floats -- BatchNorm batch
                         * statistics without a pass over C (eoe_bn_stats_partials reduces them); N % 16 == 0 */
    int32_t unpack_dw;  /* TN with gather == 1 only: C is the convolution's weight gradient in the reference's own layout
                         * [cout][cin][kh][kw] (not the [kh*kw*cin][cout] matrix): the launch goes through the workspace's partial
                         * tiles and the reduce kernel writes that order directly -- no eoe_conv_unpack_wgrad pass.  Needs the
                         * workspace (>= splits * M * N * 4 bytes, EOE_TN_WORKSPACE_BYTES always suffices for the shapes here) */
    int32_t split_k;    /* NT only, a hint: != 0 asks for the split form of a small-M problem behind a long K (M <= 1024, K >= 1536, plain or
                         * fp32-residual epilogue, no column sums): up to 8 equal k-ranges per output tile in one launch, fp32 partial tiles in the
                         * slot area of `sk_workspace` (needed: without it the hint is ignored), summed in a fixed order by a second kernel.  The split depends on K only, so a row's result
                         * does not depend on M (eoe_vit_block_fwd / _bwd ask for it on the class-token-only block's n x 768 x 3072 products:
                         * 12 tiles of 48 k-tiles are one 50-us latency chain on 12 CUs).  Ignored where it does not apply. */
    void* sk_workspace; /* NT only, optional: >= EOE_NT_STREAMK_WORKSPACE_BYTES(#CUs) bytes, 16-byte aligned, ZEROED ONCE by the caller before its
                         * first use (every launch leaves the ticket / flag words at its head zeroed again), used by one stream at a time.
                         * With it the eight-wave 256 x 256 kernel runs in its stream-K form where the tiles do not fill the CUs a whole
                         * number of times: full rounds of tiles data-parallel, the fractional last round cut along k over all CUs, fp32
                         * partial accumulators through this workspace, added in segment order by the tile's last-arriving workgroup
                         * (bitwise reproducible; no atomics on data).  A row's bits then depend on M (where the cut falls) at the level of
                         * fp32 summation order.  NULL: data-parallel tiles only. */
    int64_t sk_workspace_bytes;
} eoe_gemm_args;
/* head: 8 KiB of ticket / flag words; then two 256 x 256 fp32 partial tiles per CU */
#define EOE_NT_STREAMK_WORKSPACE_BYTES(cus) ((size_t)8192 + (size_t)(cus) * 2 * (256 * 256 * 4))
#define EOE_NT_COLSUM_WORKSPACE_BYTES(M, N) ((size_t)(((M) + 63) / 64) * (size_t)(N) * 4)

int eoe_gemm_nt(const eoe_gemm_args* args, void* stream);
int eoe_gemm_tn(const eoe_gemm_args* args, void* stream);
/* up to EOE_TN_MAX_GROUP independent TN problems with the same reduction length T, dtype, accumulate and alpha in
 * ONE launch (the four weight gradients of a transformer block fill the chip together: no split-K, no atomics) */
#define EOE_TN_MAX_GROUP 4
#define EOE_TN_WORKSPACE_BYTES (512ll * 256 * 128 * 4)   /* (#CUs rounded up) x one 256x128 fp32 tile */
#define EOE_TN_STREAMK_WORKSPACE_BYTES(cus) ((size_t)(cus) * (256 * 256 * 4))   /* one partial fp32 tile (up to 256 x 256) per CU */
int eoe_gemm_tn_grouped(const eoe_gemm_args* args, int count, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * element-wise / reduction kernels (HBM-bound; wavefront-shuffle reductions)
 * ---------------------------------------------------------------------------------------------------- */

/* fp32 [rows, cols] -> 16-bit copy [rows, cols] and (if dst_t != NULL) transposed 16-bit copy [cols, rows].
 * Produces the MFMA operand copies of the fp32 master weights once per optimiser step. */
int eoe_cast_transpose(const float* src, void* dst, void* dst_t, int rows, int cols, int dtype, void* stream);
/* the same for `count` matrices (rows, cols multiples of 4) in one launch per 56 jobs: the per-step refresh of all 16-bit
 * weight copies of a model (each matrix alone is too small to fill the chip) */
typedef struct {
    const float* src;   /* fp32 [rows, cols] */
    void* dst;          /* 16-bit [rows, cols] or NULL */
    void* dst_t;        /* 16-bit [cols, rows] or NULL */
    int32_t rows, cols;
} eoe_cast_job;
int eoe_cast_transpose_multi(const eoe_cast_job* jobs, int count, int dtype, void* stream);

/* per-channel affine + patch extraction: x fp32 [n,3,res,res] (NCHW, as the reference feeds it,
 * ad_trainer.py:411-429) -> 16-bit patch matrix [n*(res/p)^2, 3*p*p], column = c*p*p + ky*p + kx
 * (the flattened conv1 weight order, clip/model.py:207,220).  mean/std NULL = already normalised
 * (replaces transformations.py:126-138 applied at ad_trainer.py:413-425). */
int eoe_patchify(const float* x, const float* mean, const float* std, void* out, int n, int res, int patch,
                 int dtype, void* stream);

/* token assembly + ln_pre (clip/model.py:223-225): tok fp32 [n*(L-1), D] patch embeddings,
 * cls [D], pos [L, D] -> x0 fp32 [n*L, D] = cat(cls, tok) + pos (kept for backward),
 * y fp32 [n*L, D] = LayerNorm(x0) (the residual stream entering block 0), stats [n*L, 2] = (mean, rstd). */
int eoe_embed_lnpre_fwd(const float* tok, const float* cls, const float* pos, const float* gamma,
                        const float* beta, float* x0, float* y, float* stats, int n, int L, int D, float eps,
                        void* stream);
/* backward of the above: dy fp32 [n*L, D] -> dtok 16-bit [n*(L-1), D] (operand of the conv1 wgrad GEMM),
 * dcls[D] +=, dpos[L,D] +=, dgamma[D] +=, dbeta[D] += (caller zeroes or accumulates).  scratch: optional, L * 2 * D floats ->
 * dgamma / dbeta through per-token-position partial rows + a fixed-order finish kernel instead of fp32 atomics. */
int eoe_embed_lnpre_bwd(const float* dy, const float* x0, const float* stats, const float* gamma, void* dtok,
                        float* dcls, float* dpos, float* dgamma, float* dbeta, float* scratch, int n, int L, int D, int dtype,
                        void* stream);

/* LayerNorm over the last dim (clip/model.py:153-159, fp32 statistics, biased variance):
 * x fp32 [rows, D] (row stride ldx elements) -> y 16-bit [rows, D] (GEMM operand) or fp32 if out_f32,
 * stats [rows, 2].  D: any multiple of 64 from 64 to 1024, here and in eoe_layernorm_bwd / eoe_embed_lnpre_fwd / _bwd. */
int eoe_layernorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, void* y, float* stats,
                      int rows, int D, float eps, int dtype, int out_f32, void* stream);
/* dx_out[r, :] (fp32, row stride ld_out) = (dres ? dres[r, :] : 0) + LN'(dy)[r, :];  dx16 (optional) = 16-bit
 * copy of dx_out (the next GEMM's operand); dgamma/dbeta += column sums of dy*xhat / dy;  dxsum (optional) +=
 * column sums of dx_out (the bias gradient of the layer that produced the LayerNorm input's residual branch).
 * dy is 16-bit, or fp32 if dy_f32.  red_scratch: optional, EOE_LN_SCRATCH(D) floats -- the column sums then go through
 * per-workgroup partial rows and a fixed-order reduce kernel (no atomics: bitwise reproducible, and 9 us faster per call at
 * 12800 x 768) and are still ADDED to dgamma / dbeta / dxsum; NULL = fp32 atomics. */
#define EOE_LN_PARTIALS 512
#define EOE_LN_SCRATCH(D) ((size_t)EOE_LN_PARTIALS * 3 * (D))
int eoe_layernorm_bwd(const void* dy, int dy_f32, const float* x, int ldx, const float* stats,
                      const float* gamma, const float* dres, float* dx_out, int ld_out, void* dx16,
                      float* dgamma, float* dbeta, float* dxsum, float* red_scratch, int rows, int D, int dtype,
                      void* stream);

/* out[c] (+)= sum_r x[r, c]  -- bias gradients (x 16-bit [rows, cols], row stride ldx). */
int eoe_colsum(const void* x, int ldx, float* out, int rows, int cols, int dtype, int accumulate, void* stream);
/* the same sums without atomics or memset (out is overwritten): per-workgroup partial rows in `scratch`
 * (EOE_COLSUM_PARTIALS * cols floats) + a reduce kernel -- bitwise reproducible, kernels only (graph capture) */
#define EOE_COLSUM_PARTIALS 256
int eoe_colsum_det(const void* x, int ldx, float* out, float* scratch, int rows, int cols, int dtype, void* stream);

/* dst = 16-bit copy of x fp32 [rows, cols] and out[c] (+)= sum_r x[r, c] in one pass.  scratch: optional, EOE_CAST_COLSUM_PARTIALS * cols
 * floats -> the sums go through per-workgroup partial rows + a fixed-order finish kernel instead of fp32 atomics */
#define EOE_CAST_COLSUM_PARTIALS 256
int eoe_cast_colsum(const float* x, void* dst, float* out, float* scratch, int rows, int cols, int dtype, int accumulate, void* stream);

/* narrow linear head, N <= 8 outputs, exact fp32 (the 1-wide `final_linear` of CustomNet(clf=True),
 * custom_base.py:25-26, used by the BCE objective): y[M,N] = x[M,K] w[N,K]^T + bias;
 * backward: dx (optional) = dy w, dw (+)= dy^T x, db (optional) (+)= column sums of dy. */
int eoe_linear_small_fwd(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, void* stream);
int eoe_linear_small_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int M, int N,
                         int K, int accumulate, void* stream);

/* zero up to EOE_ZERO_MAX fp32 buffers in one launch (accumulators that the kernels above fill with atomics) */
#define EOE_ZERO_MAX 12
int eoe_zero_multi(float* const* ptrs, const int* counts, int n, void* stream);

/* fp32 -> 16-bit copy of n contiguous elements */
int eoe_cast(const float* src, void* dst, size_t n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * multi-head self-attention over short sequences (L <= 64, head dim 64), one wavefront per (image, head):
 *   replaces nn.MultiheadAttention(768, 12) inside ResidualAttentionBlock.attention
 *   (clip/model.py:171,181-183), without mask or dropout.
 * qkv 16-bit [n*L, 3*D] (q | k | v, each D = heads*64 wide), out 16-bit [n*L, D].
 * ---------------------------------------------------------------------------------------------------- */
int eoe_attn_fwd(const void* qkv, void* out, int n, int L, int heads, int dtype, void* stream);
/* dbias (optional, fp32 [3D]): += column sums of dqkv = the in_proj bias gradient, taken from the kernel's fp32 accumulators
 * through bias_scratch (fp32 [n, 3D], required with dbias) and a fixed-order reduce kernel -- no separate pass over dqkv */
int eoe_attn_bwd(const void* qkv, const void* dout, void* dqkv, float* dbias, float* bias_scratch, int n, int L, int heads,
                 int dtype, void* stream);
/* the same two operations for long sequences, 64 < L <= EOE_ATTN_LONG_MAX_L (ViT-B/16 at 224^2: 197 tokens, at 384^2: 577): blocks of
 * 64 queries x 64 keys with an online softmax, csrc/attention_long.hip.  Same layouts, same dbias / bias_scratch contract (the K third
 * of dbias receives exact zeros).  The forward saves nothing for the backward, which recomputes the row statistics; neither allocates;
 * two runs give the same bits.  A length outside the range, n or heads <= 0 or a dtype other than EOE_F16 / EOE_BF16 is refused before
 * any launch (eoe_attn_fwd / eoe_attn_bwd keep refusing L > 64: the caller chooses). */
#define EOE_ATTN_LONG_MAX_L 640
int eoe_attn_long_fwd(const void* qkv, void* out, int n, int L, int heads, int dtype, void* stream);
int eoe_attn_long_bwd(const void* qkv, const void* dout, void* dqkv, float* dbias, float* bias_scratch, int n, int L, int heads,
                      int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * CLIP's text tower (clip/model.py:343-356 CLIP.encode_text), forward only (the prompts are encoded once per run, under no_grad,
 * training/clip.py:59-61).
 * ---------------------------------------------------------------------------------------------------- */
/* causal multi-head attention (the -inf-above-the-diagonal mask of CLIP.build_attention_mask, model.py:284-290): key j contributes to
 * query i only when j <= i.  Same layout as eoe_attn_fwd: qkv 16-bit [n*L, 3*D] (q | k | v, D = heads*64), out 16-bit [n*L, D];
 * 1 <= L <= 128; fp32 scores and softmax.  Only rows < n*L of qkv are read and of out written. */
int eoe_attn_causal_fwd(const void* qkv, void* out, int n, int L, int heads, int dtype, void* stream);
/* token embedding (model.py:345-347): out fp32 [n*L, D] = token_embedding[tok[s, t], :] + positional_embedding[t, :].  tok [n, L] int64
 * (tok_i64 != 0, what clip.tokenize returns) or int32; token_embedding fp32 [vocab, D], positional_embedding fp32 [>= L, D].  The caller
 * checks 0 <= id < vocab (a kernel cannot report it; an id outside is clamped into the table). */
int eoe_clip_token_embed(const void* tok, int tok_i64, const float* token_embedding, const float* positional_embedding, float* out, int n,
                         int L, int D, int vocab, void* stream);
/* EOT head (model.py:349-356 before the projection): per sequence s the position t* of its largest token id (the first of equal ones:
 * text.argmax(dim=-1)), and y 16-bit [n, D] = LayerNorm(x[s*L + t*, :]) with ln_final's gamma / beta (fp32 statistics). */
int eoe_clip_eot_ln(const float* x, const void* tok, int tok_i64, const float* gamma, const float* beta, void* y, int n, int L, int D,
                    float eps, int dtype, void* stream);
/* the whole tower in one call: embedding; per layer LayerNorm-1 -> in_proj (eoe_gemm_nt) -> eoe_attn_causal_fwd -> out_proj + residual
 * -> LayerNorm-2 -> c_fc + QuickGELU -> c_proj + residual (the chain of eoe_vit_block_fwd); the EOT head; out = eot16 . text_projection.
 * Nothing is kept for a backward pass. */
typedef struct {
    int32_t n, L, D, heads, layers, vocab, embed_dim, dtype;   /* D = 64*heads, 1 <= L <= 128, D % 64 == 0 */
    float eps;
    int32_t tok_i64;
    const void* tokens;                  /* [n, L] int64 / int32 (ids checked by the caller) */
    const float* token_embedding;        /* fp32 [vocab, D] */
    const float* positional_embedding;   /* fp32 [>= L, D] */
    /* per layer: HOST arrays of `layers` device pointers; vectors fp32, matrices 16-bit row-major [out, in] */
    const float* const* ln1_g; const float* const* ln1_b; const float* const* ln2_g; const float* const* ln2_b;
    const float* const* b_in; const float* const* b_out; const float* const* b_fc; const float* const* b_proj;
    const void* const* w_in; const void* const* w_out; const void* const* w_fc; const void* const* w_proj;   /* [3D,D] [D,D] [4D,D] [D,4D] */
    const float *lnf_g, *lnf_b;          /* ln_final */
    const void* proj_t;                  /* 16-bit [embed_dim, D] = text_projection^T */
    /* caller-allocated workspace */
    float *x0, *x1;                      /* fp32 [n*L, D] residual stream (ping-pong) */
    void *xn, *qkv, *att, *hact;         /* 16-bit [n*L, D] [n*L, 3D] [n*L, D] [n*L, 4D] */
    float* stats;                        /* fp32 [n*L, 2] */
    void* eot16;                         /* 16-bit [n, D] */
    float* out;                          /* fp32 [n, embed_dim]: the text features */
    void* nt_sk_workspace;               /* optional: eoe_gemm_args.sk_workspace */
    int64_t nt_sk_workspace_bytes;
} eoe_clip_text_fwd_args;
int eoe_clip_text_fwd(const eoe_clip_text_fwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * objectives (fused heads)
 * ---------------------------------------------------------------------------------------------------- */
/* HSC (hsc.py:12-21): f fp32 [n, d]; labels int64 [n]; per sample  dist = sqrt(|f|^2+1)-1,
 * score = 1-exp(-dist), loss_i = dist if label==nominal else -log(score+1e-9);
 * loss[0] = inv_count * sum_i loss_i  (inv_count = 1/n for the plain mean, 1/global_n under data parallel).
 * Any of scores / dists / losses may be NULL. */
int eoe_hsc_fwd(const float* f, const int64_t* labels, int64_t nominal_label, float* loss, float* scores,
                float* dists, float* losses, int n, int d, float inv_count, void* stream);
/* df fp32 [n,d] = gscale[0] * inv_count * dloss_i/df (gscale = upstream gradient of the scalar loss, device
 * pointer or NULL = 1);  df16 (optional) = 16-bit copy. */
int eoe_hsc_bwd(const float* f, const int64_t* labels, int64_t nominal_label, const float* gscale, float* df,
                void* df16, int n, int d, float inv_count, int dtype, void* stream);
/* score only (hsc.py:12-15; ad_trainer.py:434-436,505) */
int eoe_hsc_score(const float* f, float* scores, int n, int d, void* stream);

/* BCE with logits (bce.py:15-20): x fp32 [n] logits; loss[0] = inv_count * sum_i bce_i; scores = sigmoid(x)
 * (1 - sigmoid if nominal_label != 0). */
int eoe_bce_fwd(const float* x, const int64_t* labels, int64_t nominal_label, float* loss, float* scores,
                float* losses, int n, float inv_count, void* stream);
int eoe_bce_bwd(const float* x, const int64_t* labels, const float* gscale, float* dx, int n, float inv_count,
                void* stream);

/* ------------------------------------------------------------------------------------------------------
 * fused multi-tensor Adam (ad_trainer.py:383: torch.optim.Adam(params, lr, weight_decay=wdk, amsgrad=False))
 * One launch over a chunk table.  Per chunk: element offset into each of the four fp32 arenas
 * (p, g, m, v may also be distinct allocations: offsets are relative to the pointers given here) and a length.
 * L2-in-gradient weight decay, bias correction per step-count group (frozen parameters, whose grad is None,
 * are simply not in the table and keep their step count: SURVEY.md section 7 "Adam details").
 * shadow16 (optional, may be NULL): 16-bit copy of the updated parameter written at the same element offset.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t p_off, g_off, m_off, v_off; /* element offsets */
    int32_t n;                          /* elements in this chunk (<= EOE_ADAM_CHUNK) */
    int32_t group;                      /* index into eoe_adam_scalars (parameters sharing a step count); | EOE_CHUNK_FP16, see eoe_sgd_multi */
} eoe_adam_chunk;
#define EOE_CHUNK_FP16 0x100            /* eoe_sgd_multi: this chunk's parameter is an fp16 tensor in the reference (clip/model.py:371-392) */
#define EOE_ADAM_CHUNK 8192
#define EOE_ADAM_GROUPS 4
typedef struct {                        /* per step-count group, computed on the host in double as torch does: */
    float step_size[EOE_ADAM_GROUPS];   /*   lr / (1 - beta1**step)                                            */
    float bc2_sqrt[EOE_ADAM_GROUPS];    /*   sqrt(1 - beta2**step)                                             */
    float grad_scale_inv;               /* the gradients are multiplied by this first (0 = 1): 1 / the loss scale of an fp16 run.
                                         * fp16's smallest subnormal is 6e-8: with 12 800 token rows sharing a mean loss the 16-bit
                                         * dY tensors of late training steps underflow, and the 10-step trajectory of the 12-layer
                                         * ViT drifts to 3e-3 off the fp32 reference; with the loss gradient scaled by 256 (the
                                         * `inv_count` argument of the loss kernels) it stays within 1.2e-4 */
} eoe_adam_scalars;

/* fused multi-tensor SGD with momentum / Nesterov = torch.optim.SGD(..., dampening=0) as constructed for CLIP models
 * (ad_trainer.py:380-381: momentum 0.9, nesterov): the same chunk tables (m_off = momentum buffer, zero-initialised; v_off unused).
 * fp16-weights mode (clip/model.py:371-392 `convert_weights`, applied by build_model :430): chunks with
 * `group & EOE_CHUNK_FP16` are updated as torch updates an fp16 parameter with an fp16 gradient -- the fp32 storage keeps
 * fp16-representable values, every elementwise op of the update rounds to fp16 (5 roundings per element, in torch's op order) */
int eoe_sgd_multi(float* p, const float* g, float* buf, const eoe_adam_chunk* chunks /*device*/, int n_chunks, float lr,
                  float momentum, float weight_decay, int nesterov, float grad_scale_inv /* as in eoe_adam_scalars; <= 0 = 1 */,
                  const int32_t* skip_flag /* device, may be NULL: see eoe_grads_nonfinite */, void* stream);
int eoe_adam_multi(float* p, const float* g, float* m, float* v, const eoe_adam_chunk* chunks /*device*/,
                   int n_chunks, const eoe_adam_scalars* scalars /*host*/, float beta1, float beta2, float eps,
                   float weight_decay, void* shadow16, int dtype, const int32_t* skip_flag /* device, may be NULL */, void* stream);
/* The same update for 2-D weights, walked by 64 x 64 tiles, which ALSO writes the two 16-bit MFMA operand copies of the new weight --
 * [rows, cols] and its transpose [cols, rows] -- that the next forward / backward multiply with (round 4).  Until then the copies were
 * made by a pass of their own before the next forward (eoe_cast_transpose_multi: the 85 M weights of the 12 blocks read again as fp32,
 * 0.14 ms per step); here they leave from the registers the update is in, through an LDS transposition.  p, m, v get exactly what
 * eoe_adam_multi writes (the same update function).  One table row per tile; rows, cols multiples of 4.  New relative to the
 * reference (torch.optim.Adam has no such copies: autocast re-casts the weights in every forward). */
typedef struct {
    int64_t p_off, g_off, m_off, v_off; /* element offsets of the MATRIX (not of the tile) from the four base pointers */
    void* d16;                          /* [rows, cols] 16-bit copy (may be NULL) */
    void* d16_t;                        /* [cols, rows] 16-bit transposed copy (may be NULL) */
    int32_t rows, cols;
    int32_t tile;                       /* this row's tile: (tile / ceil(cols / 64), tile % ceil(cols / 64)) */
    int32_t group;                      /* as in eoe_adam_chunk */
} eoe_adam_tile;
int eoe_adam_tiles(float* p, const float* g, float* m, float* v, const eoe_adam_tile* tiles /*device*/, int n_tiles,
                   const eoe_adam_scalars* scalars /*host*/, float beta1, float beta2, float eps, float weight_decay, int dtype,
                   const int32_t* skip_flag /* device, may be NULL */, void* stream);
/* Non-finite guard for the scaled fp16 step.  The reference's numerical-failure policy is the per-epoch NaN check with retry
 * (ad_trainer.py:257-280, 448-449); the loss-gradient scale this build adds for fp16 can overflow the 16-bit backward chain, so the
 * optimisers can be told to drop such a step whole.  One streaming pass over the gradients of the chunk table the optimiser is about to
 * apply.  `state` = 4 device ints {flag of even steps, flag of odd steps, steps skipped so far, steps checked so far}, zero-initialised
 * by the caller once; `parity` alternates 0 / 1 from step to step; `first` != 0 on the first chunk table of a step (several parameter
 * groups = several calls with the same parity): that call retires the previous step's flag into the skipped count.  An inf / NaN raises
 * state[parity]; pass &state[parity] as `skip_flag` to eoe_adam_multi / eoe_sgd_multi of the same step: with the flag up they touch
 * nothing (parameters, moments, 16-bit shadows).  No host synchronisation anywhere; the host reads state[2] when it cares to. */
int eoe_grads_nonfinite(const float* g, const eoe_adam_chunk* chunks /*device*/, int n_chunks, int32_t* state /*device*/, int parity,
                        int first, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * fused ViT residual block (clip/model.py:167-188 ResidualAttentionBlock.forward and its backward):
 * one call launches the whole kernel chain of a block on `stream` (no host round trips in between).
 * The attention of the block is eoe_attn_fwd / eoe_attn_bwd for L <= 64 and eoe_attn_long_fwd / eoe_attn_long_bwd above, up to
 * EOE_ATTN_LONG_MAX_L; no argument changes with the length.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, L, D, heads, dtype;   /* rows M = n*L; hidden = 4*D */
    float eps;
    /* parameters: fp32 vectors, 16-bit matrices (row-major [out, in]) and their transposes [in, out] */
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *b_in, *b_out, *b_fc, *b_proj;
    const void *w_in, *w_out, *w_fc, *w_proj;           /* [3D,D] [D,D] [4D,D] [D,4D]   */
    const void *w_in_t, *w_out_t, *w_fc_t, *w_proj_t;   /* [D,3D] [D,D] [D,4D] [4D,D]   */
    /* activations (caller-allocated; saved for backward) */
    const float* x_in;   /* fp32 [M,D] residual stream in */
    float* x_mid;        /* fp32 [M,D] after attention */
    float* x_out;        /* fp32 [M,D] residual stream out */
    void *xn1, *qkv, *att, *xn2, *hpre, *hact;   /* 16-bit [M,D] [M,3D] [M,D] [M,D] [M,4D] [M,4D] */
    float *stats1, *stats2;                      /* fp32 [M,2] */
    /* != 0: the caller reads only the class-token rows (row i*L of image i) of x_out -- the LAST block of the vision tower, whose output
     * goes through x[:, 0, :] to ln_post (clip/model.py:231-232).  The rows nobody reads are not computed: the out-projection, LayerNorm-2
     * and the MLP run on the n class-token rows, and x_mid, x_out, xn2, hpre, hact, stats2 hold [n, ...] (dense, image order) instead of
     * [n*L, ...]; xn1, qkv, att keep all rows (keys and values of every token feed the class token's attention).  Backward: dx_out is
     * fp32 [n, D]; dx_in and every parameter gradient are what the full computation gives with zero dx_out on the other rows (the
     * weight gradients to fp32 summation order: the zero rows are left out of the sums). */
    int32_t cls_only;
    /* optional: the stream-K workspace of the block's NT GEMMs (eoe_gemm_args.sk_workspace: zeroed once by the caller, one stream at a time;
     * forward and backward use the same one).  NULL: data-parallel tiles only. */
    void* nt_sk_workspace;
    int64_t nt_sk_workspace_bytes;
} eoe_vit_block_fwd_args;

/* deferred finish reductions: out[c / seg][c % seg] (+)= sum over r < R of part[r][c], c < N (blocked: eoe's [N/64][R][64] partial-row layout) */
typedef struct {
    const float* part;
    int32_t R, N, seg, blocked;
    float* out[3];
} eoe_red_job;
#define EOE_RED_TABLE_MAX 128
typedef struct eoe_red_table {
    eoe_red_job job[EOE_RED_TABLE_MAX];
    int32_t count;
    int32_t overwrite;          /* 1: out = sum, 0: out += sum (set by the first appender; all jobs of a table agree) */
} eoe_red_table;
/* launches the table's jobs (64 per launch) on `stream` and empties it */
int eoe_red_table_flush(eoe_red_table* table, void* stream);

typedef struct {
    eoe_vit_block_fwd_args f;   /* same parameters and saved activations as the forward */
    const float* dx_out;        /* fp32 [M,D] gradient wrt x_out ([n,D] with f.cls_only) */
    float* dx_in;               /* fp32 [M,D] gradient wrt x_in */
    /* parameter gradients, fp32, overwritten (or += if accumulate) */
    float *g_ln1_g, *g_ln1_b, *g_ln2_g, *g_ln2_b, *g_b_in, *g_b_out, *g_b_fc, *g_b_proj;
    float *g_w_in, *g_w_out, *g_w_fc, *g_w_proj;
    int32_t accumulate;
    /* scratch (caller-allocated, 16-bit unless noted): */
    void *d16_a;      /* [M,D]   16-bit copy of dx_out (dY of c_proj)          */
    void *d16_b;      /* [M,D]   dgrad outputs (d xn2, d att, d xn1 in turn)   */
    void *d16_c;      /* [M,D]   16-bit copy of dx_mid (dY of out_proj)        */
    void *dh;         /* [M,4D]  */
    void *dqkv;       /* [M,3D]  */
    float* dx_mid;    /* fp32 [M,D] */
    float* red_scratch; /* optional: EOE_VIT_RED_SCRATCH(n, L, D) floats -> LayerNorm-parameter and bias column sums through
                         * partial rows and fixed-order reduce kernels instead of fp32 atomics / separate passes */
    void* tn_workspace; /* optional: EOE_TN_STREAMK_WORKSPACE_BYTES(#CUs) bytes -> the grouped wgrad launch balances its 216 tiles
                         * over all CUs (eoe_gemm_args.workspace) */
    int64_t tn_workspace_bytes;
    /* Hand-over between consecutive blocks of the backward sweep (all optional; round 3).  The producer of a block's dx_out is the NEXT
     * block's LayerNorm-1 backward, which can emit what this block's first step (eoe_cast_colsum: the 16-bit copy of dx_out = dY of
     * c_proj, and its column sums = the gradient of c_proj.bias) would otherwise compute in a pass of its own:
     *   next_d16       out: 16-bit copy [n*L, D] of THIS call's dx_in, for the block that runs next in backward
     *   in_d16         in:  that copy of THIS call's dx_out, written by the previous call (a different buffer than next_d16: the
     *                       previous call's weight-gradient GEMM still reads it while this call's LayerNorm writes)
     *   in_red_scratch in:  the previous call's red_scratch (must differ from this call's: alternate two): the column sums of dx_out
     *                       sit in its LayerNorm-1 partial rows and are finished into g_b_proj by this call's one finish kernel */
    void* next_d16;
    const void* in_d16;
    const float* in_red_scratch;
    /* != 0: the four weight gradients are launched on the library's side stream and this call returns without ordering `stream` behind
     * them: the launch (216 one-per-CU workgroups, ~213 us, 40 CUs idle) then runs under the NEXT block's kernels.  The caller keeps
     * every buffer that launch reads -- dh, dqkv, d16_c, the dY of c_proj (d16_a or in_d16), the saved activations xn1 / xn2 / att / hact --
     * untouched until a later eoe_vit_block_bwd on the same stream has returned (alternate two sets of scratch; that call orders the stream
     * behind the previous launch at its own fork point) or eoe_vit_side_join(stream) was called; the weight gradients themselves may only
     * be read after eoe_vit_side_join.  Ignored (synchronous launch) while the stream is being captured or without red_scratch.
     * 2 (round 5): as 1, but a call orders the stream only behind the launch BEFORE the previous call's (the previous one is often still
     * running at this call's fork point: waiting for it stalled the compute stream ~12 us per block).  The caller then rotates THREE sets of
     * those buffers and keeps a call's buffers untouched until TWO later calls on the stream have returned (or eoe_vit_side_join). */
    int32_t async_wgrad;
    /* optional (round 5): a HOST table the block appends its finish reductions to (the five or six partial-row column sums behind its
     * bias and LayerNorm-parameter gradients) instead of launching its own finish kernel: the caller flushes the table once, after the
     * last block of the backward sweep (eoe_red_table_flush), in one or two launches for the whole tower instead of one 17-us launch per
     * block.  The caller then keeps every block's red_scratch untouched until the flush (one scratch per block, not two alternating), and
     * reads the bias / LayerNorm gradients only behind it.  NULL: the block finishes its own, as before. */
    struct eoe_red_table* red_table;
} eoe_vit_block_bwd_args;

/* floats: partial rows of the fc dgrad GEMM's fused column sums [ceil(n*L/64)][4D] + of the two LayerNorm backwards + the attention
 * backward's per-image in_proj bias sums [n][3D] (separate pieces: one kernel finishes all four at the end of the block) */
#define EOE_VIT_RED_SCRATCH(n, L, D) \
    ((size_t)(((size_t)(n) * (L) + 63) / 64) * 4 * (D) + 2 * EOE_LN_SCRATCH(D) + (size_t)(n) * 3 * (D) + (size_t)EOE_CAST_COLSUM_PARTIALS * (D))
int eoe_vit_block_fwd(const eoe_vit_block_fwd_args* a, void* stream);
int eoe_vit_block_bwd(const eoe_vit_block_bwd_args* a, void* stream);
int eoe_vit_side_join(void* stream);      /* see eoe_vit_block_bwd_args.async_wgrad */

/* ------------------------------------------------------------------------------------------------------
 * CNN backbones (cnn.py:44-86 CNN32; resnet.py:25-152 WideResNet): convolution = im2col + eoe_gemm_nt (forward),
 * eoe_gemm_tn (wgrad), eoe_gemm_nt + col2im (dgrad); BatchNorm(train statistics) + (Leaky)ReLU + MaxPool2 fused.
 * Activations between layers: 16-bit NHWC; conv outputs before BatchNorm: fp32 [n*H*W, C].
 * ---------------------------------------------------------------------------------------------------- */
/* patches [n*Ho*Wo, Kp] 16-bit, column = (ky*kw+kx)*cin + c, zero padded to Kp (multiple of 64); Ho = (H+2*pad-kh)/stride+1.
 * x_kind: 1 = the fp32 NCHW input image batch (optional per-channel normalise as ad_trainer.py:413-425),
 * 0 = a 16-bit NHWC activation, 2 = an fp32 NHWC activation. */
int eoe_im2col(const void* x, int x_kind, const float* mean, const float* std, void* out, int n, int cin, int H, int W,
               int kh, int kw, int stride, int pad, int Kp, int dtype, void* stream);
/* dx fp32 NHWC [n,H,W,C] = transpose of im2col applied to dpatches 16-bit [n*Ho*Wo, Kp] */
int eoe_col2im(const void* dpatches, float* dx, int n, int C, int H, int W, int kh, int kw, int stride, int pad, int Kp,
               int dtype, int accumulate /* dx += (a shortcut gradient already in dx) */, void* stream);
/* conv weight fp32 [cout,cin,kh,kw] -> 16-bit [cout,Kp] (patch column order), optionally its transpose [Kp,cout] and the
 * operand of the implicit stride-1 dgrad [cin, (kh*kw reversed) x cout] (dx = conv of dy with the flipped kernel);
 * and the inverse reorder of the fp32 weight gradient [cout,Kp] (or, transposed, [kh*kw*cpad, cout]) -> [cout,cin,kh,kw].
 * cpad >= cin = channels per tap in the column order (8 for the channel-padded NHWC8 image of a 3-channel first layer). */
typedef struct {      /* one eoe_conv_pack_weight call */
    const float* w;
    void *w16, *w16t, *w16d;
    int32_t cout, cin, cpad, kh, kw, Kp;
} eoe_conv_pack_job;
/* `count` weight packs in one launch per 32 jobs: the per-step refresh of all 16-bit conv weight copies of a model */
int eoe_conv_pack_weight_multi(const eoe_conv_pack_job* jobs, int count, int dtype, void* stream);
int eoe_conv_pack_weight(const float* w, void* w16, void* w16t, void* w16d, int cout, int cin, int cpad, int kh, int kw,
                         int Kp, int dtype, void* stream);
int eoe_conv_unpack_wgrad(const float* g, float* dw, int cout, int cin, int cpad, int kh, int kw, int Kp, int transposed,
                          int accumulate, void* stream);
/* 3-channel first layer without a materialised patch matrix (gather = 2 of eoe_gemm_args): the image batch fp32 NCHW
 * [n,3,H,W] (optional per-channel normalise, ad_trainer.py:413-425) becomes a 16-bit NHWC4 tensor [n,Hp,Wp,4] with the
 * convolution's zero padding made physical (pixel (h,w) at (h+pad, w+pad)); the GEMM's k axis is ky*32 + kx*4 + c with
 * K = ceil(kh/2)*64 (kw <= 8, even stride), weights packed to match, wgrad [K, cout] unpacked to [cout,3,kh,kw].
 * Needs Hp >= (Ho-1)*stride + 2*ceil(kh/2), Wp >= (Wo-1)*stride + 8, Wp even. */
int eoe_stem_pack_image(const float* x, const float* mean, const float* std, void* out, int n, int H, int W, int Hp, int Wp,
                        int pad, int cpad /* 4, or 8 = NHWC8 for gather 1 with C = 8 (any stride; pad 0: no physical border) */,
                        int dtype, void* stream);
int eoe_stem_pack_weight(const float* w, void* w16, int cout, int kh, int kw, int dtype, void* stream);
int eoe_stem_unpack_wgrad(const float* g, float* dw, int cout, int kh, int kw, void* stream);

/* batch statistics of y fp32 [M,C]: stats[0..C) = mean, stats[C..2C) = 1/sqrt(var+eps) (biased var); training updates
 * running_mean/var (momentum, unbiased var) and num_batches_tracked as nn.BatchNorm does (cnn.py:57-66); eval reads
 * the running buffers.  sums_scratch: EOE_BN_SCRATCH(C) floats, 8-byte aligned (per-workgroup partial sums, kept in double by
 * eoe_bn_stats: no atomics). */
#define EOE_BN_PARTIALS 1024
#define EOE_BN_SCRATCH(C) ((EOE_BN_PARTIALS + 3) * 2 * (C))
/* Synchronised BatchNorm for data-parallel training (the reference is single-device: its BatchNorm sees the whole batch,
 * cnn.py:57-66, resnet.py:37-41, cbam.py:74).  With a hook registered, every training-mode BatchNorm reduction point of this
 * library -- (sum, sum of squares, row count) of the forward statistics as 2C+1 doubles, (sum g, sum g*xhat, row count) of the
 * backward as 2C+1 floats -- is handed to `fn` for an in-place SUM over the ranks, on `stream`, before it is used; the row count
 * travels with the sums, so ranks may hold different numbers of rows.  fn == NULL switches back to per-rank statistics.
 * Process-wide, like eoe_set_option; not capturable in a HIP graph.  Returns 0 / the hook returns 0 on success. */
typedef int (*eoe_allreduce_fn)(void* user, void* buf, int64_t count, int is_f64, void* stream);
int eoe_set_bn_sync(eoe_allreduce_fn fn, void* user);
/* the same statistics from the partial rows [R][2][C] an eoe_gemm_nt call with `colstats` left in its workspace (R = ceil(M/64)) */
int eoe_bn_stats_partials(const float* part, int R, float* sums_scratch, float* stats, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, int M, int C, float eps, float momentum, void* stream);
int eoe_bn_stats(const float* y, float* sums_scratch, float* stats, float* running_mean, float* running_var,
                 int64_t* num_batches_tracked, int M, int C, float eps, float momentum, int training, void* stream);
/* EOE_Y16, OR-ed into the `dtype` argument of the four eoe_bn_act_* entry points below: y is not fp32 but the 16-bit (that dtype) matrix
 * an eoe_gemm_nt call with out_f32 = 0 and `colstats` wrote -- the batch statistics still come from the GEMM's fp32 accumulators; the
 * three passes that read y (forward, backward reduce, backward apply) move half the bytes.  16-bit fast mode only. */
#define EOE_Y16 0x100
/* out = maxpool_{pool}(act(bn(y))), act(z) = z > 0 ? z : slope*z (slope 0.01 = LeakyReLU of cnn.py, 0 = ReLU of
 * resnet.py, 1 = identity); y fp32 [n,H,W,C] (16-bit with EOE_Y16); out 16-bit NHWC (or fp32 if out_f32; or the reference's NCHW flatten
 * order [n, C*(H/p)*(W/p)] if nchw_flat, cnn.py:83); out16 (optional, with an fp32 NHWC out): a 16-bit copy of out, the
 * operand of the next convolution's implicit GEMM */
int eoe_bn_act_pool_fwd(const void* y, const float* stats, const float* gamma, const float* beta, void* out, void* out16,
                        int n, int H, int W, int C, int pool, int nchw_flat, int out_f32, float slope, int dtype, void* stream);
/* backward of the above: dout fp32 (layout of `out`) -> dy [n*H*W, C] 16-bit (dY operand of the conv wgrad/dgrad), or
 * fp32 if dy_f32; dgamma, dbeta.  red_scratch: EOE_BN_SCRATCH(C) floats. */
/* out[c] (+= if accumulate) = sum over the rows of an fp32 matrix [rows, C], C % 4 == 0: a convolution's bias gradient in the exact-fp32
 * mode; red_scratch: EOE_BN_SCRATCH(C) floats; fixed summation order, no atomics */
int eoe_colsum_f32(const float* x, float* out, float* red_scratch, int rows, int C, int accumulate, void* stream);
int eoe_bn_act_pool_bwd(const void* y, const float* stats, const float* gamma, const float* beta, const float* dout,
                        float* red_scratch, void* dy, int dy_f32, float* dgamma, float* dbeta, int n, int H, int W, int C,
                        int pool, int nchw_flat, int training, int accumulate, float slope, int dtype, void* stream);

/* BatchNorm + activation + OVERLAPPING MaxPool2d(k, stride, pad) in one pass (the stem of resnet.py:93-96: the
 * 112x112x64 post-ReLU activation is never written): out fp32 [n,Ho,Wo,C], optional 16-bit copy, idx = winning tap;
 * backward: dout fp32 [n,Ho,Wo,C] -> dy 16-bit [n*H*W, C] (gather form; fp32 with dtype = EOE_F32), dgamma, dbeta;
 * red_scratch EOE_BN_SCRATCH(C). */
int eoe_bn_act_maxpool_fwd(const void* y, const float* stats, const float* gamma, const float* beta, float* out, void* out16,
                           uint8_t* idx, int n, int H, int W, int C, int k, int stride, int pad, float slope, int dtype,
                           void* stream);
int eoe_bn_act_maxpool_bwd(const void* y, const float* stats, const float* gamma, const float* beta, const float* dout,
                           const uint8_t* idx, float* red_scratch, void* dy, float* dgamma, float* dbeta, int n, int H, int W,
                           int C, int k, int stride, int pad, int training, float slope, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Resize and ColorJitter of the input pipeline (N1; main/train_imagenet.py:30-31 Resize(256), main/train_clip_imagenet.py:28-29
 * Resize((256,256)) + ColorJitter(0.01 x 4), main/train_cifar.py:32, CLIP's clip_official/clip/clip.py:58-65 bicubic Resize(224)).
 * The reference runs them on PIL images (torchvision -> Pillow); these reproduce Pillow's 8-bit arithmetic byte for byte.
 *   eoe_resize_coeffs   HOST helper: Pillow's antialiased filter taps for one axis (Resample.c), 22-bit fixed point.
 *                       bounds int32 [out_size][2] = (first source index, taps); kk int32 [out_size][ksize_cap].
 *                       bounds == NULL or kk == NULL: only *ksize_out (taps per output) is returned.
 *   eoe_resize_pass_u8  one separable pass over uint8 data viewed as [outer, axis_in, inner] -> [outer, axis_out, inner]
 *                       (bounds / kk on the DEVICE): horizontal pass outer = n*H, inner = 3; vertical pass outer = n,
 *                       inner = Wo*3.  Image.resize = horizontal, then vertical, each skipped when the size is unchanged.
 *   eoe_color_jitter_u8 dst[slot] = ColorJitter of src[idx[slot]] (uint8 NHWC [., H, W, 3]): factors fp32 [n][4] =
 *                       (brightness, contrast, saturation around 1; hue around 0) as torchvision samples them, order int32
 *                       [n][4] = the permutation in which the four ops (0..3) are applied; an entry outside 0..3 skips.
 *                       gray_mean_scratch: n int32.
 * ---------------------------------------------------------------------------------------------------- */
enum { EOE_RESIZE_BILINEAR = 2, EOE_RESIZE_BICUBIC = 3 };   /* PIL.Image.BILINEAR / BICUBIC */
int eoe_resize_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int ksize_cap, int* ksize_out);
int eoe_resize_pass_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* kk, int ksize, int64_t outer,
                       int axis_in, int axis_out, int inner, void* stream);
int eoe_color_jitter_u8(const uint8_t* src, int64_t n_src, const int32_t* idx, const float* factors, const int32_t* order,
                        int32_t* gray_mean_scratch, uint8_t* dst, int n, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Multi-scale modes (MSM): the reference's label-conditioned input filters (utils/transformations.py: GpuDFTLowPassFilter,
 * GpuDFTHighPassFilter with their MinMaxNorm, Blur = kornia gaussian_blur2d with reflect borders) on fp32 NCHW images in the
 * [0, 1] pixel scale.  magnitude <= 0 is a bit copy.  lpf / hpf need square images; blur takes k = max(min(2*int(m/2) + 1,
 * 2*(W/2) - 1), 3) taps, sigma = m, and refuses k > 223 (EOE_ERR_UNSUPPORTED; every k of images up to 224 wide is taken).
 *   eoe_msm_operator   HOST helper, fp64: the 1-D operator G of lpf (A) / hpf (B) for side n at `magnitude` (e = min(m, n/2)).
 *                      rank_limited = 0: re / im are the dense n x n G (row-major), *cols_out = n, cs_out = {0, 1}.
 *                      rank_limited = 1: G = cs_out[0] I + cs_out[1] U U^H; re / im are U, n x r row-major, *cols_out = r
 *                      (r <= n/2).  re == NULL or im == NULL: only *cols_out / cs_out (either may be NULL).
 *   eoe_msm_workspace  which operator form eoe_msm_filter reads (EOE_MSM_FORM_*) and the workspace bytes it needs
 *   eoe_msm_filter     y[i] = filter(x[i]) for rows[i] != 0 (rows: n_img uint8 on the DEVICE, NULL = every row), y[i] = x[i] bit
 *                      for bit otherwise; out of place.  oper (DEVICE, fp32): FORM_DENSE = [Re G | Im G] as two n x n blocks;
 *                      FORM_RANK = [Ut (n x 2r) | Ut^T (2r x n)] with Ut[j] = (Re U[j][0..r), Im U[j][0..r)); FORM_NONE: unused.
 *                      The workspace is caller-owned device memory; launches go to `stream`.
 * ---------------------------------------------------------------------------------------------------- */
enum { EOE_MSM_LPF = 1, EOE_MSM_HPF = 2, EOE_MSM_BLUR = 3 };
enum { EOE_MSM_FORM_NONE = 0, EOE_MSM_FORM_DENSE = 1, EOE_MSM_FORM_RANK = 2 };
int eoe_msm_operator(int op, int n, int magnitude, int rank_limited, double* re, double* im, int* cols_out, double* cs_out);
int eoe_msm_workspace(int op, int n_img, int C, int H, int W, int magnitude, int* form_out, size_t* bytes_out);
int eoe_msm_filter(int op, const float* x, float* y, const uint8_t* rows, int n_img, int C, int H, int W, int magnitude,
                   const float* oper, void* workspace, size_t workspace_bytes, void* stream);
/* The sharpen MSM: Pillow's ImageFilter.UnsharpMask(radius, percent, threshold) (the reference's PilUnsharpMask: radius 2,
 * percent int(magnitude * 100), threshold 3), byte-exact with Pillow: 3 horizontal + 3 vertical box passes with replicated edges
 * on uint8, then |d| > threshold ? clamp(src + d * percent / 100) : src per pixel with d = src - blurred.  One launch; rows as in
 * eoe_msm_filter (NULL = every image, unselected images bit copies); percent == 0 is a bit copy; out of place; C is 1 or 3;
 * planes of at most 65536 pixels; 0 <= radius <= 256, 0 <= percent <= 2^20.
 *   eoe_msm_sharpen_u8   uint8 NHWC [n_img, H, W, C] (PIL images, resident sets)
 *   eoe_msm_sharpen_f32  fp32 NCHW [n_img, C, H, W] in [0, 1]: sharpens q = clamp(rint(x * 255)) and writes q' / 255.0f
 *                        (ToTensor's bits: exact for batches on the k / 255 grid)
 *   eoe_crop_flip_u8     the crop / flip of eoe_augment_batch (same params, zero padding, both flip orders) on its own:
 *                        uint8 NHWC [n, Ho, Wo, 3] out, the image a PIL-stage filter sees before ToTensor */
int eoe_msm_sharpen_u8(const uint8_t* src, uint8_t* dst, const uint8_t* rows, int n_img, int H, int W, int C, float radius,
                       int percent, int threshold, void* stream);
int eoe_msm_sharpen_f32(const float* x, float* y, const uint8_t* rows, int n_img, int C, int H, int W, float radius, int percent,
                        int threshold, void* stream);
int eoe_crop_flip_u8(const uint8_t* src, int64_t n_src, int Hs, int Ws, const int32_t* params, uint8_t* out, int n, int Ho, int Wo,
                     int flip_first, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Per-task input normalisation: the reference's 'normalize' / 'gcn-normalize' transform strings (datasets/bases.py:293-372).
 *   eoe_set_moments_u8  the statistics pass over a resident uint8 NHWC set [n_src, H, W, C] (C = 1 or 3), one launch.  index:
 *                       n_index int64 rows of the set on the DEVICE (NULL = rows 0 .. n_index - 1).  All outputs are exact
 *                       integers (int64, DEVICE): chan_sums [n_index][C][2] = per channel (sum v, sum v^2); img_stats
 *                       [n_index][3] = per image over all channels (min v, max v, sum |N v - S|) with N = C*H*W and S = sum v
 *                       over the image, so the image's mean absolute deviation in the [0, 1] scale is that sum / (255 N^2).
 *                       A row outside [0, n_src) reads nothing and gets -1 in all its outputs.  Integer sums: independent of
 *                       the reduction order, bitwise repeatable.  The host turns them into the reference's RunningStats
 *                       recurrence / GCN extremes (eoe_amd/normalize.py).
 *   eoe_gcn_normalize   global contrast normalisation (utils/transformations.py:326-349) and the per-channel Normalize that
 *                       follows it, fp32 NCHW [n, C, H, W] (C = 1 or 3): y = ((x - mean_i) / scale_i - shift[c]) / range[c],
 *                       mean_i over the N = C*H*W features of sample i, scale_i = mean |x - mean_i| (EOE_GCN_L1) or
 *                       sqrt(sum (x - mean_i)^2) / N (EOE_GCN_L2).  shift / range: C floats each on the DEVICE, both or
 *                       neither (NULL, NULL = GCN alone).  y == x (in place) is allowed and gives the same bits; partial
 *                       overlap is not.  No epsilon: a constant sample gives non-finite values, as in the reference.  One
 *                       launch, fixed summation order (fp64 sums), no atomics.
 * ---------------------------------------------------------------------------------------------------- */
enum { EOE_GCN_L1 = 1, EOE_GCN_L2 = 2 };
int eoe_set_moments_u8(const uint8_t* src, int64_t n_src, int H, int W, int C, const int64_t* index, int64_t n_index,
                       int64_t* chan_sums, int64_t* img_stats, void* stream);
int eoe_gcn_normalize(const float* x, float* y, int n, int C, int H, int W, int scale, const float* shift, const float* range,
                      void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Candidate search of the evolutionary OE-sample experiment (evolve/__init__.py:100-157: the squared distances of a pool of
 * candidate images to the parent image(s) and their sorted order), on a resident uint8 image set [n_set][D] (D = H*W*C bytes per
 * image, any layout: both sides of a difference are read the same way).
 *   eoe_pool_sqdist_u8   out[k][p] = sum_e (set[query_idx[k]][e] - set[cand_idx[p]][e])^2, exact int64 [K][P] on the DEVICE.
 *                        query_idx / cand_idx are HOST arrays (K <= 1024, P <= 2^20 rows; repeats allowed, a query may be a
 *                        candidate): they are checked against n_set before anything is launched (EOE_ERR_ARG, nothing is read)
 *                        and copied into the workspace on `stream`, so they must stay valid until the stream has passed the call.
 *                        Every candidate is read from memory once and compared with all K queries.  D is split over workgroups
 *                        (chunks of 1 KiB .. 64 KiB, about 1 024 workgroups); a chunk sums in 32 bits, chunks are added in 64 bits
 *                        by a second small launch (no atomics; integer sums, so bitwise repeatable either way).  D % 16 != 0
 *                        takes a byte-wise path.  workspace: eoe_pool_sqdist_workspace(D, K, P) bytes, 16-byte aligned.
 *   eoe_pool_sqdist_ragged_u8   the same sum for a set of MIXED sizes (arena / offsets / sizes / n_set / C: the ragged set of
 *                        eoe_ragged_crop_flip_u8 below; arena_bytes: its length; the arena starts at and is as long as a multiple of
 *                        16 bytes), over a crop_h x crop_w x C window of each listed image:
 *                        out[k][p] = sum (window(query[k]) - window(cand[p]))^2.  query [K][3] / cand [P][3] are HOST int32 arrays of
 *                        (row, top, left), the origin relative to the row's own unpadded image; window bytes outside the image count
 *                        as 0 (any origin is allowed: every window row and column is checked against the device `sizes`, and an
 *                        image whose extent does not lie in the arena counts as empty).  Rows are checked against n_set, K <= 1024,
 *                        P <= 2^20 and 1 <= crop_h * crop_w * C <= 2^26 before anything is copied or launched (EOE_ERR_ARG).  Chunks,
 *                        32-bit partial sums and the 64-bit second pass are those of eoe_pool_sqdist_u8: no atomics, bitwise
 *                        repeatable.  Window rows are not aligned; no load leaves [arena, arena + arena_bytes).  Lists that lie back
 *                        to back on the host (cand == query + 3 K) are uploaded in one copy; they must stay valid until the stream
 *                        has passed the call.  workspace: eoe_pool_sqdist_ragged_workspace(...) bytes, 16-byte aligned.
 *   eoe_pool_rank        order[k][.] = the stable ascending order of dist[k][.] as positions 0 .. P-1 (equal distances keep list
 *                        order: the `arg` of torch's stable sort), int32 [K][P], DEVICE; dist int64 [K][P].  One launch, rank by
 *                        counting in LDS.  P <= 1024, larger P is EOE_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------------------- */
int eoe_pool_sqdist_workspace(int64_t D, int K, int P, size_t* bytes_out);
int eoe_pool_sqdist_u8(const uint8_t* set, int64_t n_set, int64_t D, const int32_t* query_idx, int K, const int32_t* cand_idx, int P,
                       int64_t* out, void* workspace, size_t workspace_bytes, void* stream);
int eoe_pool_sqdist_ragged_workspace(int crop_h, int crop_w, int C, int K, int P, size_t* bytes_out);
int eoe_pool_sqdist_ragged_u8(const uint8_t* arena, int64_t arena_bytes, const int64_t* offsets, const int32_t* sizes, int64_t n_set,
                              int C, int crop_h, int crop_w, const int32_t* query, int K, const int32_t* cand, int P, int64_t* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int eoe_pool_rank(const int64_t* dist, int K, int P, int32_t* order, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Data-parallel exchange (new -- the reference is single-device, main/__init__.py:110-114): gradient
 * SUM all-reduce and score / label all-gather over RCCL on xGMI, one process per GPU.  RCCL is bound at run time (the librccl
 * already in the process, else the system one); without it these return EOE_ERR_UNSUPPORTED and nothing else is affected.
 * Rank 0 makes the id (eoe_comm_unique_id) and hands its EOE_COMM_ID_BYTES bytes to the other ranks by any out-of-band channel
 * (the launcher's store); every rank then calls eoe_comm_init.  The `_async` calls run on the communicator's own side stream
 * behind everything `after_stream` holds at the time of the call (overlap with the rest of backward); eoe_comm_join makes
 * `stream` wait for all collectives issued so far.  Buffers are caller-owned device memory.
 * dtype: EOE_F32 | EOE_F16 | EOE_BF16 | EOE_COMM_I64.  algo: EOE_COMM_ALGO_RING = RCCL's all-reduce; EOE_COMM_ALGO_RS_AG =
 * in-place reduce-scatter + all-gather (count %% world == 0, else the former): on a fully connected xGMI node every rank
 * exchanges 1/world of the buffer with every peer at once instead of walking a ring.
 * ---------------------------------------------------------------------------------------------------- */
#define EOE_COMM_ID_BYTES 128
enum { EOE_COMM_I64 = 8 };
enum { EOE_COMM_ALGO_RING = 0, EOE_COMM_ALGO_RS_AG = 1 };
typedef struct eoe_comm* eoe_comm_t;
int eoe_comm_unique_id(void* id_out);
int eoe_comm_init(const void* id, int rank, int world, int device, eoe_comm_t* out);
int eoe_comm_destroy(eoe_comm_t comm);
int eoe_comm_info(eoe_comm_t comm, int* rank, int* world);
int eoe_comm_allreduce_sum_async(eoe_comm_t comm, void* buf, int64_t count, int dtype, int algo, void* after_stream);
int eoe_comm_allgather_async(eoe_comm_t comm, const void* send, void* recv, int64_t send_count, int dtype, void* after_stream);
int eoe_comm_join(eoe_comm_t comm, void* stream);
/* synchronised BatchNorm over this communicator without leaving the library: registers (enable != 0) or clears an eoe_set_bn_sync
 * hook that sums the BatchNorm reduction buffers with ncclAllReduce IN the stream the BatchNorm kernels run on (no side stream: the
 * very next kernel consumes the sums).  The sums use a SECOND RCCL communicator over the same ranks (bucket all-reduces of the first one
 * may be in flight on the side stream); `bn_id` is its id -- EOE_COMM_ID_BYTES bytes from eoe_comm_unique_id() on rank 0, identical on
 * every rank, handed over like the first one's (NULL once the communicator has it, and with enable == 0).  The library allocates no
 * device memory and synchronises nothing here.  The communicator must outlive the registration. */
int eoe_comm_sync_bn(eoe_comm_t comm, int enable, const void* bn_id);

/* ------------------------------------------------------------------------------------------------------
 * Parity mode (SURVEY.md section 7 "Hard parts", section 8d "Parity run"): the convolutions / linear layers of the BatchNorm
 * encoders (cnn.py:73-86, resnet.py:85-149) in plain fp32 -- fp32 activations and fp32 master weights as operands, one fp32 FMA
 * per product in a fixed order, no 16-bit rounding.  Since round 3 on the fp32 matrix cores (v_mfma_f32_16x16x4_f32; the
 * register-tiled SGEMM on the vector ALUs stays selectable: option "parity_flags" bit 0): the conformant mode of BASELINE configs 1-3
 * and the instrument that tells the fast path's 16-bit operand rounding from an implementation difference.
 *   x: fp32 NHWC [n,H,W,C], or the fp32 NCHW image batch if x_nchw (then optional per-channel Normalize (x - mean) / std,
 *   ad_trainer.py:413-425); w: [cout, C, kh, kw] (the nn.Conv2d parameter itself; a Linear layer is H = W = kh = kw = 1);
 *   y / dy: fp32 [n*Ho*Wo, cout]; dx: fp32 NHWC (+= if accumulate); dw: [cout, C, kh, kw] overwritten (slab sums in fixed
 *   order: bitwise reproducible).  geo.C = input channels; geo.Ho / geo.Wo must match the geometry.
 *   workspace (forward / dgrad; may be NULL / 0): with few output tiles and a long reduction (small maps, FC layers) the reduction
 *   is cut into slabs whose partial outputs ([slab][rows][cout] floats) go here and are summed in slab order; a workspace of
 *   k x the output size allows k slabs.  A stride-2 dgrad over an even map runs as four parity-class GEMMs (no work on taps a pixel
 *   never meets); "parity_flags" bit 1 turns that off.
 * ---------------------------------------------------------------------------------------------------- */
/* the 3-channel NCHW image batch, optionally normalised ((x - mean) / std, ad_trainer.py:413-425), as an fp32 NHWC map with 4 channels
 * (the 4th = 0): with it (geo.C = 4, weights zero-padded to [cout, 4, kh, kw]) the first layer runs through the float4 paths of
 * eoe_conv_f32_fwd / _wgrad instead of element-wise gathers */
int eoe_pack_image_nhwc4(const float* x_nchw, const float* mean, const float* stdv, float* out_nhwc4, int n, int H, int W, void* stream);
/* w_kmajor (forward / dgrad; may be NULL): the k-major fp32 copy of w made by eoe_conv_f32_pack_weights (forward: wf, dgrad: wd) -- the
 * kernels then stage the weight tile with 16-byte loads and stores instead of scalar gathers with a stride of kh * kw floats (+5-10 %) */
int eoe_conv_f32_pack_weights(const float* w /* [cout, cin, kh, kw] */, float* wf /* [kh*kw*cin, cout] or NULL */,
                              float* wd /* [kh*kw*cout, cin] or NULL */, int cout, int cin, int kh, int kw, void* stream);
int eoe_conv_f32_fwd(const float* x, int x_nchw, const float* mean, const float* stdv, const float* w, const float* bias, float* y,
                     const eoe_conv_geometry* geo, int cout, void* workspace, size_t workspace_bytes, const float* w_kmajor, void* stream);
int eoe_conv_f32_dgrad(const float* dy, const float* w, float* dx, const eoe_conv_geometry* geo, int cout, int accumulate,
                       void* workspace, size_t workspace_bytes, const float* w_kmajor, void* stream);
size_t eoe_conv_f32_wgrad_workspace(const eoe_conv_geometry* geo, int cout);
int eoe_conv_f32_wgrad(const float* x, int x_nchw, const float* mean, const float* stdv, const float* dy, float* dw,
                       const eoe_conv_geometry* geo, int cout, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * WideResNet + CBAM (resnet.py:85-109,130-149; cbam.py:31-107).  All activations fp32 NHWC.  The 7x7/2 stem,
 * the 3x3 and the 1x1/2 downsample convolutions are eoe_im2col + eoe_gemm_nt (+ eoe_bn_stats / eoe_bn_act_pool_*
 * with slope 0 = ReLU or 1 = none); the pieces below are the HBM-bound rest of a BasicBlock.
 * ---------------------------------------------------------------------------------------------------- */
/* nn.MaxPool2d(k, stride, pad) (resnet.py:96): out [n,Ho,Wo,C]; idx [n,Ho,Wo,C] = winning tap ky*k+kx (first maximum) */
int eoe_maxpool_fwd(const float* x, float* out, void* out16 /* optional 16-bit copy */, uint8_t* idx, int n, int H, int W, int C,
                    int k, int stride, int pad, int dtype, void* stream);
int eoe_maxpool_bwd(const float* dout, const uint8_t* idx, float* dx, int n, int H, int W, int C, int k, int stride, int pad,
                    void* stream);

/* ChannelGate (cbam.py:31-66, pool_types avg+max): out = x * sigmoid(mlp(avgpool x) + mlp(maxpool x)),
 * mlp = Linear(C, Ch) -> ReLU -> Linear(Ch, C).  The forward fills the saved tensors the backward reads. */
typedef struct {
    const float* x;       /* [n, HW, C] */
    float* out;           /* [n, HW, C] (forward only) */
    const float* w1;      /* mlp.1.weight [Ch, C] */
    const float* b1;      /* mlp.1.bias   [Ch]    */
    const float* w2;      /* mlp.3.weight [C, Ch] */
    const float* b2;      /* mlp.3.bias   [C]     */
    float* pooled;        /* [n, 2, C]  avg, max       (saved) */
    int* argmax;          /* [n, C]     position of the max (saved) */
    float* hidden;        /* [n, 2, Ch] post-ReLU      (saved) */
    float* scale;         /* [n, C]     sigmoid output (saved) */
    int n, HW, C, Ch;
} eoe_cgate_args;
typedef struct {
    eoe_cgate_args f;
    const float* dout;    /* [n, HW, C] */
    float* dx;            /* [n, HW, C] */
    float* dscale;        /* [n, C]     scratch */
    float* dpooled;       /* [n, 2, C]  scratch */
    float* dhidden;       /* [n, 2, Ch] scratch */
    float *dw1, *db1, *dw2, *db2;      /* written (not accumulated) */
} eoe_cgate_bwd_args;
int eoe_cgate_fwd(const eoe_cgate_args* a, void* stream);
int eoe_cgate_bwd(const eoe_cgate_bwd_args* a, void* stream);

/* SpatialGate (cbam.py:76-92): out = x * sigmoid(bn(conv7x7([max_c x, mean_c x]))), conv 2->1 without bias, pad 3,
 * BatchNorm2d(1) with the module's eps / momentum (cbam.py:14: momentum 0.01) and running buffers. */
typedef struct {
    const float* x;       /* [n, H, W, C] */
    float* out;           /* [n, H, W, C] (forward only) */
    const float* w;       /* spatial.conv.weight [1, 2, 7, 7] */
    const float* gamma;   /* spatial.bn.weight [1] or NULL */
    const float* beta;    /* spatial.bn.bias   [1] or NULL */
    float* running_mean;  /* [1] or NULL */
    float* running_var;   /* [1] or NULL */
    int64_t* num_batches_tracked;   /* [1] or NULL */
    float* comp;          /* [n, H, W, 2] channel max, channel mean (saved) */
    int* argmax;          /* [n, H, W]    channel of the max        (saved) */
    float* z;             /* [n, H, W]    conv output               (saved) */
    float* stats;         /* [2]          mean, rstd used           (saved) */
    float* scale;         /* [n, H, W]    sigmoid output            (saved) */
    float* sums;          /* EOE_BN_SCRATCH(1) floats scratch */
    int n, H, W, C;
    float eps, momentum;
    int training;         /* 1: batch statistics (+ running update), 0: running statistics */
    const float* res;     /* optional (forward): residual [n, H, W, C]; then out = relu(x * scale + res), the block's junction
                           * (resnet.py:143-147) fused into the gate's last pass */
    void* out16;          /* optional with res: 16-bit copy of out (operand of the next convolution) */
    int dtype;            /* EOE_F16 | EOE_BF16 of out16 */
} eoe_sgate_args;
#define EOE_SGATE_PARTIALS 512
#define EOE_SGATE_RED (2 + 2 * EOE_SGATE_PARTIALS)
typedef struct {
    eoe_sgate_args f;
    const float* dout;    /* [n, H, W, C] */
    float* dx;            /* [n, H, W, C] */
    float* dscale;        /* [n, H, W]    scratch */
    float* dcomp;         /* [n, H, W, 2] scratch */
    float* red;           /* [EOE_SGATE_RED] scratch: per-workgroup partial sums of the 1-channel BatchNorm backward */
    float* dw;            /* [1, 2, 7, 7] written */
    float* dgamma;        /* [1] or NULL */
    float* dbeta;         /* [1] or NULL */
    float* wpart;         /* [n, 98] scratch: per-image partial sums of dw (added up in a fixed order: no atomics) */
} eoe_sgate_bwd_args;
int eoe_sgate_fwd(const eoe_sgate_args* a, void* stream);
int eoe_sgate_bwd(const eoe_sgate_bwd_args* a, void* stream);
/* A BasicBlock's tail out = relu(SpatialGate(ChannelGate(x)) + res) (resnet.py:143-147, cbam.py:100-106) as ONE unit: the channel-gated
 * tensor is never written (every consumer multiplies x by the channel scale on the fly -- the same fp32 product), the junction's ReLU mask
 * is applied where the gradient is first read, and the spatial gate's input gradient feeds the channel gate's reduction and its final
 * pass without being stored: 22 + 32 bytes per activation element instead of 30 + 44.  cg / cb: the channel gate's argument blocks
 * (cg->out unused); sg / sb: the spatial gate's (sg->x, sb->dout, sb->dx unused; sg->res, sg->out, sg->out16 required / as in eoe_sgate_fwd).
 * backward: dout = gradient at the block's output, out = that output (the mask); g (written) = the residual branch's gradient,
 * cb->dx = the gradient of x; cb->dscale must hold EOE_CBAM_DSCALE_SLICES slices of [n, C] and sb->dcomp FOUR floats per pixel here (scale, dcomp0, dcomp1, argmax bits: one 16-byte record). */
#define EOE_CBAM_DSCALE_SLICES 8
int eoe_cbam_junction_fwd(const eoe_cgate_args* cg, const eoe_sgate_args* sg, void* stream);
int eoe_cbam_junction_bwd(const eoe_cgate_bwd_args* cb, const eoe_sgate_bwd_args* sb, const float* dout, const float* out, float* g,
                          void* stream);
/* The data-only form of eoe_cbam_junction_bwd (an explanation: no parameter requires a gradient): g and dx as above, bit for bit, and
 * nothing else.  cg / sg are the FORWARD argument blocks as saved (cg->out, sg->x, sg->out, sg->res, sg->out16, the running buffers and
 * sg->sums unused); the scratch: dscale EOE_CBAM_DSCALE_SLICES slices of [n, C], dpooled [n, 2, C], dhidden [n, 2, Ch], dsp [n, H, W],
 * dcomp [n, H, W, 4], red EOE_SGATE_RED floats (untouched unless sg->training).  No parameter gradient is written and no
 * weight-gradient kernel is launched, so the map is not capped at (H + 6)(W + 6) <= 8192; with sg->training == 0 the BatchNorm takes its
 * running statistics and the batch-mean reduction is not launched either. */
int eoe_cbam_junction_bwd_data(const eoe_cgate_args* cg, const eoe_sgate_args* sg, const float* dout, const float* out, float* g, float* dx,
                               float* dscale, float* dpooled, float* dhidden, float* dsp, float* dcomp, float* red, void* stream);

/* out = relu(a + b) (resnet.py:146-147); g = dout * [out > 0] (the gradient of both summands) */
int eoe_add_relu_fwd(const float* a, const float* b, float* out, void* out16 /* optional 16-bit copy */, int dtype,
                     int64_t count, void* stream);
int eoe_relu_bwd(const float* dout, const float* out, float* g, int64_t count, void* stream);
/* nn.AvgPool2d over the whole HW grid (resnet.py:38,104): pooled_scratch [n,2,C] receives (mean, max), the mean is
 * pooled_scratch[:,0,:]; backward dx[n,hw,c] = dout[n,c] / HW */
int eoe_avgpool_fwd(const float* x, float* pooled_scratch, int* argmax_scratch, int n, int HW, int C, void* stream);
int eoe_avgpool_bwd(const float* dout, float* dx, int n, int HW, int C, void* stream);

/* the other objectives of the reference's TRAINER registry (training/__init__.py:8-11), same
 * conventions as eoe_hsc_* / eoe_bce_* (loss[0] = inv_count * sum of the per-sample losses; gscale = upstream gradient):
 *   DSAD  (dsad.py:17-21):  loss_i = |f|^2 if label == nominal else 1 / (|f|^2 + 1e-9);  score = the HSC score (eoe_hsc_score)
 *   DSVDD (dsvdd.py:24-27): loss_i = score_i = |f - center|^2 (center fp32 [d], from prepare_metric dsvdd.py:10-22)
 *   focal (focal.py:11-36): b = bce_with_logits(x, y), pt = clamp(exp(-b), eps, 1 - eps), loss_i = (1 - pt)^gamma * b;
 *                           scores = sigmoid(x) (1 - sigmoid if nominal_label != 0) */
/* Epoch-tail metrics on the device (ad_trainer.py:452-455,517-521): out[0] = ROC AUC (tie-averaged rank
 * statistic = sklearn's trapezoidal area), out[1] = average precision (sklearn's step-wise sum), both fp64, NaN when a class is
 * missing; scores fp32 [n], labels int64 [n] (positive_label = the anomalous label, 1); computed from exact integer pair counts
 * (n^2 compares, no sort).  scratch: EOE_AUC_SCRATCH_BYTES(n) bytes. */
#define EOE_AUC_SCRATCH_BYTES(n) ((size_t)(((n) + 255) / 256) * 24)
int eoe_auc_ap(const float* scores, const int64_t* labels, int64_t positive_label, double* out, void* scratch, int n, void* stream);
/* The curves behind those two numbers (ad_trainer.py:453, 517, 520: sklearn's roc_curve and precision_recall_curve; the containers
 * logger.py:36-91 keep them).  For the K distinct scores thr_0 > thr_1 > ... > thr_{K-1}:
 *     out_tps[k] = #{j: labels[j] == positive_label, scores[j] >= thr_k},   out_fps[k] = #{j: scores[j] >= thr_k} - out_tps[k]
 * exact integers, from pair counts (n^2 compares, no sort, no atomics); out_thr[k] carries the bits of the element with the smallest
 * index among its equal scores (what a reversed stable sort keeps; -0.0 == 0.0 is one group).  out_roc_* hold the same table without
 * the slots roc_curve's drop_intermediate removes: when drop_intermediate != 0 and K > 2, slot k with 0 < k < K-1 stays iff the second
 * difference of fps or of tps at k is not 0; otherwise the whole table.  out_counts[0] = K, out_counts[1] = K_roc.  The rates
 * (fps / fps[K-1], tps / tps[K-1], tps / (tps + fps)) are left to the caller.
 *   scores fp32 [n], labels int64 [n]; out_fps / out_tps / out_roc_fps / out_roc_tps int64 [n], out_thr / out_roc_thr fp32 [n] (the
 *   first K resp. K_roc entries are written), out_counts int32 [2]; all DEVICE, no two of them overlapping.  1 <= n <= 2^20.
 *   Non-finite scores are the caller's to reject (NaN compares false with everything; nothing is written out of range).
 *   scratch: eoe_rank_curves_scratch_bytes(n) bytes (0 for an n outside the range), 4-byte aligned.  Four enqueues on `stream`
 *   (a memset and three launches); K stays on the device in between. */
size_t eoe_rank_curves_scratch_bytes(int n);
int eoe_rank_curves(const float* scores, const int64_t* labels, int64_t positive_label, int n, int drop_intermediate,
                    int64_t* out_fps, int64_t* out_tps, float* out_thr, int64_t* out_roc_fps, int64_t* out_roc_tps, float* out_roc_thr,
                    int32_t* out_counts, void* scratch, void* stream);
/* The epoch's score histograms (ad_trainer.py:458-465, 541-546: SummaryWriter.add_histogram on the scores of label 0 and of label 1;
 * csrc/hist.hip): for both label groups in one pass, what np.histogram(values, bins=edges) counts and the five scalars TensorBoard
 * stores with it.  Bin b = [edges[b], edges[b+1]), the last bin closed on both sides, a value outside [edges[0], edges[E-1]] in no
 * bin; scores are compared as float64 against the table (a binary search; -0.0 is 0.0).
 *   scores fp32 [n] DEVICE; labels int64 [n] DEVICE: group 0 = label 0, group 1 = label 1, any other label in neither group;
 *   labels NULL: every score is in group 0 and group 1 is empty.  n >= 1.
 *   edges_host / edges: the same float64 table [E] in HOST memory (checked here: finite, strictly ascending) and in DEVICE memory
 *   (read by the kernel; the caller uploads it once per device).  2 <= E <= 4001 (the table and both groups' counters share LDS).
 *   out_counts int32 [2][E-1] DEVICE (cleared here); out_stats fp64 [2][5] DEVICE, 8-byte aligned: per group count, min, max, sum and
 *   sum of squares over ALL of the group's scores, binned or not; an empty group reports count 0 and zeros.
 *   Counts are integer adds (LDS atomics per workgroup, integer atomics into out_counts); the fp64 sums use no floating-point atomic
 *   and a fixed order: two runs give the same bits.  Non-finite scores are the caller's to reject (they land in no bin).
 *   scratch: eoe_score_hist_scratch_bytes(n) bytes (0 for n < 1), 8-byte aligned, may be dirty.  Three enqueues on `stream` (a memset
 *   and two launches). */
size_t eoe_score_hist_scratch_bytes(int n);
int eoe_score_hist(const float* scores, const int64_t* labels, int n, const double* edges_host, const double* edges, int E,
                   int32_t* out_counts, double* out_stats, void* scratch, void* stream);
/* The extremes of the scores (csrc/topk.hip): per label group the k highest and the k lowest scores and where they stand -- the false
 * alarms and misses of an evaluation (the reference ranks OE individuals this way, evolve/tree.py scores_best / imsave_best).
 * Groups as in eoe_score_hist: group 0 = label 0, group 1 = label 1, any other label in neither; labels NULL: every score in group 0.
 * End 0 ("most") is descending by score, equal scores by ascending position: np.argsort(-s, kind="stable")[:k] over the group's
 * members; end 1 ("least") ascending by score, equal scores by ascending position: np.argsort(s, kind="stable")[:k].  -0.0 == 0.0.
 *   scores fp32 [n], labels int64 [n] or NULL; out_idx int32 [2 groups][2 ends][k]: positions in `scores`; out_val fp32 [2][2][k]: the
 *   selected elements' own bits; out_counts int32 [3]: the sizes m_0, m_1 of the groups and the number of non-finite scores among
 *   their members.  All DEVICE.  Only the first min(k, m_g) slots of a list are written, the others stay as the caller left them.
 *   When out_counts[2] != 0 the lists are unspecified (nothing is written out of range).  1 <= n <= 2^20, 1 <= k <= 1024.
 *   A radix select over distinct 52-bit integer keys (ordered score image, position) and a sort of the at most 1 024 selected keys in
 *   LDS: integer compares and integer adds only, no n^2 pass, two runs give the same bytes.
 *   scratch: eoe_score_extremes_scratch_bytes(n, k) bytes (0 for an n or k outside the ranges), 16-byte aligned, may be dirty.  Eight
 *   enqueues on `stream` (a memset and seven launches); the thresholds stay on the device in between. */
size_t eoe_score_extremes_scratch_bytes(int n, int k);
int eoe_score_extremes(const float* scores, const int64_t* labels, int n, int k, int32_t* out_idx, float* out_val, int32_t* out_counts,
                       void* scratch, void* stream);
/* The per-class breakdown of the scores (csrc/breakdown.hip): which class causes the misses.  Sample j has the dense class id
 * class_ids[j] in [0, K) and the side side_per_class[class_ids[j]] (0 nominal, 1 anomalous; data.ad_targets).  The sub-problem of class
 * k is class k against the pool of all samples of the other side, label 1 on the anomalous side; row K is the pooled problem (every
 * anomalous sample against every nominal one).  The threshold of a problem is the score of the positive whose group of equal scores
 * holds place m among the positives in descending order (gt < m <= ge; the bits of the group's smallest index; -0.0 == 0.0), where m
 * is the caller's: m_per_class[k] for an anomalous class (its positives are the class), m_pooled for row K and for every nominal class
 * (their positives are the whole anomalous side).  An m outside [1, number of positives] leaves the slot as cleared.
 *   out_counts int64 [K+1][4], row k = { 2U, fps, tps, n_k }:
 *       2U  = sum over (positive p, negative q) of 2 [s_p > s_q] + [s_p == s_q]: ROC AUC = 2U / (2 n_pos n_neg); row K: 0
 *       fps = #{negatives: s >= threshold}, tps = #{positives: s >= threshold};  n_k = the size of class k; row K: 0
 *   out_ap fp64 [K]: an anomalous class's average precision (1 / n_k) sum over p in k of ge_own(p) / (ge_own(p) + ge_pool(p)), ge_x(p) =
 *       #{j in x: s_j >= s_p}; a fixed summation order (two runs give the same bits); 0 for a nominal class (not built: it would take a
 *       count per (pool sample, class)) and for a class without samples.
 *   out_thr fp32 [K+1]: the thresholds (a nominal class's is row K's).  Rows without a writer read as 0: the caller knows the class
 *       sizes and reports a problem with an empty side as NaN.
 *   scores fp32 [n], class_ids int32 [n], side_per_class uint8 [K], m_per_class int32 [K]: all DEVICE, as are the outputs; 4-byte
 *   aligned (out_counts, out_ap: 8-byte).  1 <= n <= 2^20, 1 <= K <= 1024, 0 <= m_pooled <= n.  A sample whose class id is outside
 *   [0, K) is in no class and no pool.  Non-finite scores are the caller's to reject (nothing is written out of range).
 *   Exact integer pair counts (n^2 compares over cdiv(n, 256) workgroups, no sort, no atomics), then one workgroup per class.
 *   scratch: eoe_class_breakdown_scratch_bytes(n, K) bytes (0 for an n or K outside the ranges), 4-byte aligned, may be dirty.  Four
 *   enqueues on `stream` (two memsets of the outputs and two launches); the thresholds stay on the device in between. */
size_t eoe_class_breakdown_scratch_bytes(int n, int K);
int eoe_class_breakdown(const float* scores, const int32_t* class_ids, const uint8_t* side_per_class, const int32_t* m_per_class,
                        int m_pooled, int n, int K, int64_t* out_counts, double* out_ap, float* out_thr, void* scratch, void* stream);
/* DeLong's estimator of the covariance of K ROC AUCs measured on the same n samples, as exact integer sums (csrc/delong.hip).
 * Positives: label 1 (m of them); negatives: label 0 (n0); any other label is in neither.  Per column k of scores and per sample
 *       a[k,i] = 2 #{j negative: s_k[i] > s_k[j]} + #{j negative: s_k[i] == s_k[j]}   (positive i)
 *       b[k,j] = 2 #{i positive: s_k[i] > s_k[j]} + #{i positive: s_k[i] == s_k[j]}   (negative j)
 * with IEEE fp32 compares (-0.0 == 0.0, the infinities are ordinary values).  With P = K (K + 1) / 2:
 *   out int64 [2K + 2P + 3] = { T_pos[K], T_neg[K], A[P], B[P], m, n0, nan }:
 *       T_pos[k] = sum_i a[k,i] and T_neg[k] = sum_j b[k,j]: equal by construction, both written so that the caller can check;
 *           ROC AUC_k = T[k] / (2 m n0)
 *       A[k,l] = sum_i a[k,i] a[l,i], B[k,l] = sum_j b[k,j] b[l,j] for k <= l, the upper triangle row by row
 *       nan = the number of NaN scores among the positives and negatives of all columns; when it is not 0 the sums are unspecified
 *           (a NaN compares false; nothing is written out of range)
 *   Every entry stays below 2^63: A, B <= 16 n^3 / 27 (4.4e14 at n = 90 000, 6.9e17 at n = 2^20).
 *   scores fp32 [K][n] (column k at scores + k n), labels int64 [n], out: all DEVICE; 4-byte aligned (labels, out: 8-byte).
 *   2 <= n <= 2^20, 1 <= K <= 8.  Integer compares and adds only (the atomics are integer adds): two runs give the same bytes.
 *   scratch: eoe_delong_scratch_bytes(n, K) bytes (0 for an n or K outside the ranges), 4-byte aligned, may be dirty.  Four enqueues
 *   on `stream` (a memset and three launches); m and n0 stay on the device in between.
 * eoe_delong_slices: into how many slices the count pass cuts the opposite side at (n, K) (0 outside the ranges); rows and scores
 *   are handled in blocks and tiles of 256. */
size_t eoe_delong_scratch_bytes(int n, int K);
int eoe_delong_slices(int n, int K);
int eoe_delong_counts(const float* scores, const int64_t* labels, int n, int K, int64_t* out, void* scratch, void* stream);
/* The stratified, paired bootstrap of AUC, AP and FPR at a TPR level, resampled and counted on the device (csrc/bootstrap.hip).
 * Positives: label 1 (m of them); negatives: label 0 (n0); any other label is in neither.  Each stratum is numbered in ascending sample
 * index.  Replicate b draws m times with replacement from the positives and n0 times from the negatives, and all K columns share the draws:
 *   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32)
 *   and counter (j, b, stratum, 0), stratum 0 for the negatives and 1 for the positives, gives the draws 4j .. 4j+3 of that (replicate,
 *   stratum); the unused words of the last call are dropped; a word w selects position (w * size) >> 32 of its stratum (multiply-shift
 *   without rejection: a position's probability is off by less than size / 2^32).
 * With c[i] the multiplicity of sample i in replicate b, per column k (IEEE fp32 compares: -0.0 == 0.0, the infinities are ordinary values):
 *   out_u2  int64 [K][B+1] sum over (positive i, negative j) of c[i] c[j] (2 [s_i > s_j] + [s_i == s_j]); the AUC is u2 / (2 m n0)
 *   out_fps int64 [K][B+1] sum over negatives j of c[j] [s_j >= t], t the score at place p of the resampled positives in descending order
 *                         with multiplicity, p the smallest integer with p / m >= tpr in float64; the FPR is fps / n0
 *   out_ap  f64   [K][B+1] sum over the distinct scores in descending order of (tps_g - tps_{g-1}) / m * (tps_g / (tps_g + fps_g)) with the
 *                         weighted cumulative counts: sklearn's average_precision_score of the resample.  Summed in a fixed order (within
 *                         about n 2^-53 of any other order).
 *   Entry [k][b] belongs to replicate b < B; entry [k][B] is the same number on the full sample (every multiplicity 1), so that the
 *   point estimates need no second pass over the scores.
 *   counts  int32 [3] = { m, n0, the number of NaN scores among the positives and negatives of all columns }; when the last is not 0 the
 *                         tables are unspecified (nothing is read or written out of range).  With m == 0 or n0 == 0 the tables are zeros.
 * u2 and fps are exact integers and all three tables are the same bytes on every run: integer LDS atomics, no floating-point atomics.
 *   scores fp32 [K][n] (column k at scores + k n), labels int64 [n], the outputs: all DEVICE; 4-byte aligned (labels, tables: 8-byte).
 *   2 <= n <= 2^20, 1 <= K <= 8, 1 <= B <= 65536, 0 < tpr <= 1.
 *   scratch: eoe_bootstrap_scratch_bytes(n, K, B) bytes (0 outside the ranges; it does not grow with B), 8-byte aligned, may be dirty.
 *   Five enqueues on `stream` (a memset and four launches).  A workgroup of the replicate pass counts EOE_BOOTSTRAP_CHUNK sorted
 *   positions at a time in LDS and regenerates its draws once per chunk.
 * eoe_bootstrap_draws: the multiplicities of replicate b per sample, out int32 [n] (0 for an ignored label), for tests and diagnosis;
 *   0 <= b < 65536; scratch: eoe_bootstrap_scratch_bytes(n, 1, 1) bytes; a memset and two launches. */
#define EOE_BOOTSTRAP_CHUNK 16384
size_t eoe_bootstrap_scratch_bytes(int n, int K, int B);
int eoe_bootstrap_counts(const float* scores, const int64_t* labels, int n, int K, int B, uint64_t seed, double tpr, int64_t* out_u2,
                         int64_t* out_fps, double* out_ap, int32_t* counts, void* scratch, void* stream);
int eoe_bootstrap_draws(const int64_t* labels, int n, int b, uint64_t seed, int32_t* out, void* scratch, void* stream);
/* Nearest neighbours in feature space (csrc/knn.hip): for every row of q the k rows of r with the smallest squared Euclidean distance,
 * ascending by distance, equal distances by ascending reference index -- np.argsort(d2_row, kind="stable")[:k] -- each with its distance.
 *   q fp32 [nq, D] with row stride ldq, r fp32 [nr, D] with row stride ldr (ldq, ldr >= D; nothing is read past column D of a row);
 *   idx int32 [nq, k], d2 fp32 [nq, k], counts int32 [2] = { non-finite query rows, non-finite reference rows }.  All DEVICE, 4-byte
 *   aligned; a 16-byte aligned base with ld % 4 == 0 takes 16-byte loads, anything else element loads with the same result.
 *   d2 = (|q|^2 + |r|^2) - 2 q.r, clamped at 0, the dot product a k-ordered fp32 fmaf chain (v_mfma_f32_32x32x2_f32): within
 *   (2 D + 8) 2^-24 (|q|^2 + |r|^2) of the exact distance.  The nq x nr matrix is never stored: a workgroup reduces 128 queries x 1 024
 *   references to k keys (ordered distance bits, reference index) per query in LDS, a second kernel merges a query's chunks.
 *   Fewer than k eligible references: the tail holds idx = -1, d2 = +inf.  A reference row that holds a NaN or an infinity is never
 *   returned; a query row that holds one gets idx = -1, d2 = NaN throughout.
 *   1 <= k <= 64, 1 <= D <= 2048, 0 <= nr < 2^24, nq >= 0; nq == 0 returns 0 without a launch (counts is then left alone).
 *   EOE_ERR_ARG, naming the argument, before any launch otherwise.  Integer compares only behind the distance, no atomics: two runs
 *   give the same bytes.
 *   scratch: eoe_feature_knn_scratch_bytes(nq, nr, D, k) bytes (0 outside the ranges), 16-byte aligned, may be dirty.  Three launches
 *   on `stream`. */
size_t eoe_feature_knn_scratch_bytes(int nq, int nr, int D, int k);
int eoe_feature_knn(const float* q, int ldq, const float* r, int ldr, int nq, int nr, int D, int k, int* idx, float* d2, int* counts,
                    void* scratch, void* stream);
/* The Gaussian baseline in feature space (csrc/mahalanobis.hip): the moments a mean and a Ledoit-Wolf covariance are made of, and the
 * squared Mahalanobis distance.  Both matrix products are k-ordered fp32 fmaf chains (v_mfma_f32_32x32x2_f32).
 * eoe_feature_moments: x fp32 [n, D] with row stride ld (ld >= D; nothing is read past column D of a row).  A row that holds a NaN or an
 *   infinity is excluded; over the rows used:
 *     counts int32 [2] = { rows used, rows excluded }
 *     mean fp32 [D]    = column sum / rows used: the sum in float64 in a fixed order, the quotient rounded once to fp32
 *     scatter f64 [D, D] = Z^T Z with z = x - mean formed in fp32 (no centred copy of x is stored): the rows are cut into slices, a
 *         slice's sum is an fp32 fmaf chain in row order, the slices are added in ascending order in float64.  Only the 128 x 128 tiles
 *         on or above the diagonal are computed, the lower half is their mirror image: symmetric bit for bit.  Each entry lies within
 *         (n + 4) 2^-24 sum_i |z_ia z_ib| of the exact sum over the fp32 z.
 *     m4 f64 [1]       = sum_i (|z_i|^2)^2; |z_i|^2 in fp32, one wave per row: an fmaf chain per lane over columns lane, lane + 64, ...,
 *         then the wave's butterfly sum (relative error (ceil(D / 64) + 6) 2^-24 to first order); squared and added in float64 in a
 *         fixed tree over the rows' positions
 *   No row used (n == 0 included): mean, scatter and m4 are zeros.  The number of slices is a pure function of (n, D), chosen so that
 *   tiles x slices is about 256 workgroups; the fp32 partial tiles in scratch take 26 MB at most, whatever n.
 *   All DEVICE; x, mean, counts 4-byte aligned, scatter and m4 8-byte aligned; a 16-byte aligned x with ld % 4 == 0 takes 16-byte loads,
 *   anything else element loads with the same result.  0 <= n <= 2^30, 1 <= D <= 2048.  Six launches on `stream`.
 * eoe_mahalanobis_score: d2[i] = sum_j y_ij^2 with y_ij = sum_k W[j,k] (x[i,k] - mean[k]); x fp32 [nq, D] (row stride ldx), mean fp32 [D],
 *   W fp32 [P, D] (row stride ldw; ldx, ldw >= D): the inverse Cholesky factor of the covariance (P == D) or any P directions.
 *   d2 fp32 [nq]; count int32 [1] = query rows that hold a NaN or an infinity, whose d2 is NaN.  x - mean is formed in fp32 while a
 *   tile is staged; y is never stored: a workgroup squares and adds 128 queries x 128 rows of W in registers, one fp32 partial per
 *   (query, 128 rows of W) goes to scratch and a last kernel adds a query's partials in ascending order.  Within
 *   2^-24 (2 (D + 2) sum_j |y_j| a_j + (P + 2) sum_j y_j^2), a_j = sum_k |W[j,k]| |x_k - mean_k|, of the exact value of the fp32 inputs.
 *   lower != 0 (accepted only with P == D) promises W[j,k] == 0 for k > j and skips those k-steps; while every fp32 x - mean is finite (0 * z == 0) the bytes are
 *   those of lower == 0.  1 <= D, P <= 2048, 0 <= nq <= 2^30; nq == 0 returns 0 without a launch (count is then left alone).  Three launches.
 * Both: EOE_ERR_ARG, naming the argument, before any launch; no atomics, fixed orders: two runs give the same bytes.
 *   scratch: eoe_feature_moments_scratch_bytes(n, D) / eoe_mahalanobis_score_scratch_bytes(nq, D, P) bytes (0 outside the ranges),
 *   16-byte aligned, may be dirty. */
size_t eoe_feature_moments_scratch_bytes(int n, int D);
int eoe_feature_moments(const float* x, int ld, int n, int D, float* mean, double* scatter, double* m4, int* counts, void* scratch,
                        void* stream);
size_t eoe_mahalanobis_score_scratch_bytes(int nq, int D, int P);
int eoe_mahalanobis_score(const float* x, int ldx, int nq, int D, const float* mean, const float* W, int ldw, int P, int lower, float* d2,
                          int* count, void* scratch, void* stream);
/* Greedy k-center (farthest-point) coreset of the rows of x (csrc/coreset.hip): idx[0] = start; idx[t], t >= 1, is the eligible, not yet
 * chosen row with the largest squared distance to its nearest centre among idx[0 .. t-1], equal distances to the LOWEST row;
 * radius[t] is that squared distance, radius[0] = +inf.  A chosen row is never chosen again (m == n: a permutation of the finite rows).
 *   x fp32 [n, D] with row stride ldx >= D (nothing is read past column D of a row); idx int32 [m], radius fp32 [m], assign int32 [n],
 *   d2min fp32 [n], counts int32 [2].  All DEVICE, 4-byte aligned; a 16-byte aligned x with ldx % 4 == 0 and D % 4 == 0 takes 16-byte loads,
 *   anything else element loads with the same bytes in every output.
 *   assign[i] = the position t of row i's nearest centre, the earliest chosen one on equal distances (updated only on strictly
 *   smaller); d2min[i] = that squared distance; a centre has its own position and 0.
 *   A row that holds a NaN or an infinity is never a centre: assign = -1, d2min = NaN.  counts[0] = the number of such rows; counts[1] = 1
 *   if `start` is one of them, and then every other output is unspecified.  Fewer than m eligible rows: the tail holds idx = -1,
 *   radius = NaN.
 *   Distance: sum_d (x_d - c_d)^2 in the difference form in fp32 -- each lane an fmaf chain over its columns in ascending order, then
 *   the wave's butterfly sum: a fixed order, at most D + 2 roundings on any term, so relative error at most g = (D + 2) 2^-24 /
 *   (1 - (D + 2) 2^-24); exact on integer-valued features while the sums stay below 2^24.
 *   m launches chained on `stream`, one streaming pass over x per centre; the next centre's index stays on the device (an integer
 *   atomicMax of (ordered distance bits, 0xFFFFFFFF - row) per workgroup), the host neither waits nor reads inside the call.  No
 *   float atomics: two runs give the same bytes.
 *   1 <= D <= 2048, 1 <= n < 2^24, 1 <= m <= n, 0 <= start < n; EOE_ERR_ARG, naming the argument, before any launch otherwise.
 *   scratch: eoe_feature_coreset_scratch_bytes(n, D, m) bytes (0 outside the ranges), 16-byte aligned, may be dirty. */
size_t eoe_feature_coreset_scratch_bytes(int n, int D, int m);
int eoe_feature_coreset(const float* x, int ldx, int n, int D, int m, int start, int* idx, float* radius, int* assign, float* d2min,
                        int* counts, void* scratch, void* stream);

/* CLIP text-prompt objective (training/clip.py:66-103): f fp32 [n, d] image features, text fp32 [T, d]
 * (2 <= T <= 64; the frozen, l2-normalised text features prepare_metric returns, clip.py:50-64), l = 100 * f/|f| . text^T;
 *   loss_i = -log_softmax(l)[pick]: pick = T-1 for the anomalous label (1 - nominal), 0 for the nominal label (one_vs_rest) or
 *   the arg max over j < T-1 (leave_one_out); other labels contribute 0;  scores = softmax(l)[:, T-1] (any of scores / loss NULL).
 * eoe_clip_score: the same score for text rows the caller has l2-normalised (compute_anomaly_score, clip.py:66-79). */
int eoe_clip_fwd(const float* f, const float* text, const int64_t* labels, int64_t nominal_label, int leave_one_out, float* loss,
                 float* scores, float* losses, int n, int d, int T, float inv_count, void* stream);
int eoe_clip_bwd(const float* f, const float* text, const int64_t* labels, int64_t nominal_label, int leave_one_out,
                 const float* gscale, float* df, int n, int d, int T, float inv_count, void* stream);
int eoe_clip_score(const float* f, const float* text, float* scores, int n, int d, int T, void* stream);
int eoe_dsad_fwd(const float* f, const int64_t* labels, int64_t nominal_label, float* loss, float* losses, int n, int d,
                 float inv_count, void* stream);
int eoe_dsad_bwd(const float* f, const int64_t* labels, int64_t nominal_label, const float* gscale, float* df, int n, int d,
                 float inv_count, void* stream);
int eoe_dsvdd_fwd(const float* f, const float* center, float* loss, float* dists, int n, int d, float inv_count, void* stream);
int eoe_dsvdd_bwd(const float* f, const float* center, const float* gscale, float* df, int n, int d, float inv_count,
                  void* stream);
int eoe_focal_fwd(const float* x, const int64_t* labels, int64_t nominal_label, float* loss, float* scores, float* losses,
                  int n, float inv_count, float gamma, float eps, void* stream);
int eoe_focal_bwd(const float* x, const int64_t* labels, const float* gscale, float* dx, int n, float inv_count, float gamma,
                  float eps, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * on-device input pipeline: gather + RandomCrop (zero padding) + RandomHorizontalFlip +
 * ToTensor + Gaussian noise + per-channel Normalize in one pass over a uint8 NHWC image set resident in HBM
 * (main/train_cifar.py:31-38, main/train_clip_imagenet.py:27-36, training/ad_trainer.py:413-425).
 *   src    uint8 [n_src, Hs, Ws, 3];   params int32 [n, 4] = (source index, crop top, crop left, flip) per batch slot
 *          (top / left may be negative or reach past the image: RandomCrop(padding) with fill 0)
 *   out    fp32 NCHW [n, 3, Ho, Wo] = ((src / 255 + noise_std * N(0,1)) - mean[c]) / std[c]   (mean/std NULL: none)
 *   flip_first 1: flip the source then crop (CIFAR order), 0: crop then flip (CLIP order)
 *   noise  element e = (c*Ho + y)*Wo + x of slot b draws Box-Muller from splitmix64(seed*2^40 + b*2^18 + e)
 * ---------------------------------------------------------------------------------------------------- */
int eoe_augment_batch(const uint8_t* src, int64_t n_src, int Hs, int Ws, const int32_t* params, const float* mean,
                      const float* std, float* out, int n, int Ho, int Wo, int flip_first, float noise_std, uint64_t seed,
                      void* stream);
/* The same pipeline for C = 1 or 3 channels (C = 1: the 28 x 28 tasks, main/train_fmnist.py:31-38, main/train_mnist.py), and
 * Grayscale(1), the first transform of the Fashion-MNIST chain, for the resident colour OE set.
 *   eoe_augment_batch_c  eoe_augment_batch on src uint8 [n_src, Hs, Ws, C] -> fp32 NCHW [n, C, Ho, Wo]; mean / std hold C floats.
 *                        The noise rule is unchanged: with C = 1 the element is e = y*Wo + x, the draws of channel 0 of the
 *                        3-channel form.  C = 3 is eoe_augment_batch itself.  With C = 1 a slot whose source index lies outside
 *                        [0, n_src) reads nothing and comes out as padding.
 *   eoe_crop_flip_u8_c   eoe_crop_flip_u8 on [n_src, Hs, Ws, C] -> uint8 [n, Ho, Wo, C], C = 1 or 3
 *   eoe_grayscale_u8     dst[p] = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of the n_pixels RGB pixels of src (uint8, 3 bytes per
 *                        pixel -> 1 byte per pixel): Pillow's Image.convert("L"), byte for byte.  Out of place; any alignment
 *                        (16-byte aligned pointers take the 16-pixels-per-thread path).  Deterministic: convert a resident set once. */
int eoe_augment_batch_c(const uint8_t* src, int64_t n_src, int Hs, int Ws, int C, const int32_t* params, const float* mean,
                        const float* std, float* out, int n, int Ho, int Wo, int flip_first, float noise_std, uint64_t seed,
                        void* stream);
int eoe_crop_flip_u8_c(const uint8_t* src, int64_t n_src, int Hs, int Ws, int C, const int32_t* params, uint8_t* out, int n, int Ho,
                       int Wo, int flip_first, void* stream);
int eoe_grayscale_u8(const uint8_t* src, uint8_t* dst, int64_t n_pixels, void* stream);
/* CLIP's own preprocessing INSIDE the train chain (main/train_clip_cifar.py:26-35, train_clip_fmnist.py:27-36, train_clip_mnist.py:25-29):
 *   RandomCrop(S, padding) / RandomHorizontalFlip -> Resize(n_px, BICUBIC) -> CenterCrop(n_px) -> convert("RGB") -> ToTensor -> noise
 *   -> Normalize.  The upsample follows the random crop, so it runs per sample per step: one launch does the whole chain.
 *   eoe_augment_resize_batch  src uint8 [n_src, Hs, Ws, C] (C = 1 or 3), params as eoe_augment_batch -> out fp32 NCHW [n, 3, n_px, n_px]:
 *       the crop_h x crop_w crop of eoe_crop_flip_u8_c (zero padding, both flip orders; a slot whose index lies outside
 *       [0, n_src) is all padding), Pillow's horizontal then vertical pass crop -> n_px on uint8 (the arithmetic of
 *       eoe_resize_pass_u8; the horizontal result is rounded to uint8 first), the byte repeated to three channels when C = 1, then
 *       out = ((v / 255 + noise_std * N(0,1)) - mean[c]) / std[c] with the noise rule of eoe_augment_batch on element
 *       e = (c*n_px + y)*n_px + x; mean / std hold 3 floats (or both NULL).
 *       bounds / kk: the DEVICE copies of eoe_resize_coeffs(crop, n_px, filter) with ksize_cap = its ksize (3 bilinear, 5 bicubic);
 *       the caller uploads them once per (crop, n_px, filter) and keeps them.
 *       EOE_ERR_ARG before any launch: crop_h != crop_w (CenterCrop is then no identity), crop > 64, n_px > 256, n_px < crop
 *       (downscaling), a filter other than EOE_RESIZE_BILINEAR / EOE_RESIZE_BICUBIC, 3*n_px*n_px >= 2^18, n >= 2^22, seed >= 2^24. */
int eoe_augment_resize_batch(const uint8_t* src, int64_t n_src, int Hs, int Ws, int C, const int32_t* params, int crop_h, int crop_w,
                             int n_px, int filter, const int32_t* bounds, const int32_t* kk, const float* mean, const float* std,
                             float* out, int n, int flip_first, float noise_std, uint64_t seed, void* stream);
/* Image sets of MIXED sizes (main/train_imagenet.py:30-34, train_cub.py, train_dtd.py, train_mvtec.py, train_custom.py: Resize(256)
 * with an int keeps the aspect ratio, so after it every image has its own shape).  A ragged set is
 *   arena   uint8, the images back to back, each row-major HWC with C = 1 or 3 for the whole set; no row is assumed aligned
 *   offsets int64 [n_src], the byte at which image i starts;   sizes int32 [n_src, 2] = (H_i, W_i)
 * all three on the device.  params / out / flip_first / noise / mean / std are those of the functions above, and the results are
 * equal to theirs bit for bit on each image taken as a 1-image set; a slot whose index lies outside [0, n_src) is all padding.
 * n == 0 returns 0 without a launch.
 *   eoe_ragged_augment_batch         eoe_augment_batch_c: fp32 NCHW [n, C, Ho, Wo]
 *   eoe_ragged_crop_flip_u8          eoe_crop_flip_u8_c: uint8 [n, Ho, Wo, C]
 *   eoe_ragged_color_jitter_crop_u8  eoe_color_jitter_u8 of image params[slot][0] as a whole (C = 3), THEN eoe_crop_flip_u8 of it,
 *                                    uint8 [n, Ho, Wo, 3], without writing the jittered image: one pass sums the gray level in
 *                                    front of the contrast op over the slot's whole image into gray_mean_scratch (int32 [n]), the
 *                                    second applies the ops under the crop window only; the padding stays 0
 *   eoe_ragged_resize_pass_u8        eoe_resize_pass_u8 for every image of a set in one launch: image i is src + offs[2 i] as
 *                                    [outer, axis_in, inner] -> dst + offs[2 i + 1] as [outer, axis_out, inner] (offs int64 [n, 2]),
 *                                    desc int32 [n, 8] = (outer, axis_in, axis_out, inner, bounds_at, kk_at, ksize, first) where
 *                                    bounds_at / kk_at are positions in `taps`, an int32 array holding the eoe_resize_coeffs
 *                                    tables (ksize_cap = ksize) of every distinct (in, out) of the set; an image whose axis is at
 *                                    its target already has ksize = 0 and is copied (Pillow skips that pass).  max_out_bytes: the
 *                                    largest image's output, which sizes the launch.  All arrays on the device; the taps are
 *                                    computed on the host.
 *                                    first: a window on the output axis (CenterCrop behind Resize, clip_official/clip/clip.py:
 *                                    58-65).  The pass writes outputs [first, first + axis_out) of the FULL output axis, packed as
 *                                    [outer, axis_out, inner]; bounds_at / kk_at name the tables of the full axis, whose row
 *                                    first + x is output x; a ksize = 0 pass copies positions [first, first + axis_out) of
 *                                    axis_in.  first = 0 with axis_out the full axis is the whole pass, bit for bit what it was
 *                                    before the field had a meaning.  offs[2 i] is signed: behind a horizontal pass that wrote only
 *                                    source rows [r0, r1) the vertical pass (outer = 1) is given the start of the intermediate minus
 *                                    r0 rows, and its taps, all within [r0, r1), land inside it.  The descriptors live on the
 *                                    device, so the window is checked where it is made, on the host (data.ragged_resize_plan:
 *                                    first < 0 or first + count beyond the full axis is a ValueError before any launch). */
int eoe_ragged_augment_batch(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src, int C,
                             const int32_t* params, const float* mean, const float* std, float* out, int n, int Ho, int Wo,
                             int flip_first, float noise_std, uint64_t seed, void* stream);
int eoe_ragged_crop_flip_u8(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src, int C,
                            const int32_t* params, uint8_t* out, int n, int Ho, int Wo, int flip_first, void* stream);
int eoe_ragged_color_jitter_crop_u8(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src,
                                    const int32_t* params, const float* factors, const int32_t* order, int32_t* gray_mean_scratch,
                                    uint8_t* out, int n, int Ho, int Wo, int flip_first, void* stream);
int eoe_ragged_resize_pass_u8(const uint8_t* src, uint8_t* dst, const int64_t* offs, const int32_t* desc, const int32_t* taps, int n,
                              int64_t max_out_bytes, void* stream);

/* Image grids composed on the device (csrc/grid.hip): the uint8 picture the reference's Logger.logimg hands to cv2.imwrite
 * (utils/logger.py:202-295), from images that already lie in HBM.  n cells in `groups` pictures of per = n / groups cells each, back to
 * back in `out`; one picture is uint8 [Hg + sep_height, Wg, 3]:
 *     cell = h x w, or maxres x maxres when h > maxres or w > maxres (torch's bilinear rule, align_corners=False, no antialias)
 *     xmaps = min(nrow, per), ymaps = ceil(per / xmaps), Hg = (ch + pad) * ymaps + pad, Wg = (cw + pad) * xmaps + pad
 *     cell k at (pad + (k / xmaps) * (ch + pad), pad + (k % xmaps) * (cw + pad)); padding and unused cells 0; C = 1 fills 3 channels
 *     sep_height > 0: that many black rows in front of row min((ch + pad) * sep_at + pad / 2, Hg)
 * table  DEVICE int32 [n, 4] = (row of the source set, window top, window left, mark); a row outside [0, n_src) is an all-zero cell.
 *        top / left are read by the ragged form only.  mark: -1, or the frame colour 0xRRGGBB (read only when `marked`).
 * marked == 0: make_grid(normalize=True, scale_each=True) per cell over its values after the resize:
 *        byte = trunc((clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5f) * 255)
 * marked != 0: logger.py:234-246: byte = trunc((x - lo) / (hi - lo) * 255), 0 for a constant cell, and the outermost 1-pixel frame
 *        of a cell whose mark >= 0 is that colour.
 * minmax DEVICE float [2 n] scratch (the per-cell min / max, left there).  out_bytes must be the pictures' size exactly.  n == 0 with
 * out_bytes == 0 returns 0 without a launch.  EOE_ERR_ARG, naming the argument, before any launch: C not 1 or 3, nrow < 1, pad / maxres /
 * sizes out of range, n * C * ch * cw or out_bytes at or beyond 2^31.
 *   eoe_grid_f32        x fp32 NCHW [n_src, C, h, w]: the values as they are
 *   eoe_grid_u8         set uint8 NHWC [n_src, H, W, C]: value = byte / 255.0f (ToTensor)
 *   eoe_grid_ragged_u8  the crop_h x crop_w window at (top, left) of image `row` of a ragged set (arena / offsets / sizes as above),
 *                       relative to the unpadded image; window pixels outside the image are 0 (the windows eoe_pool_sqdist_ragged_u8
 *                       compares); an image whose extent does not lie in [0, arena_bytes) is all 0 */
int eoe_grid_f32(const float* x, int64_t n_src, int C, int h, int w, const int32_t* table, int n, int groups, int nrow, int pad,
                 int maxres, int sep_height, int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes, void* stream);
int eoe_grid_u8(const uint8_t* set, int64_t n_src, int H, int W, int C, const int32_t* table, int n, int groups, int nrow, int pad,
                int maxres, int sep_height, int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes, void* stream);
int eoe_grid_ragged_u8(const uint8_t* arena, int64_t arena_bytes, const int64_t* offsets, const int32_t* sizes, int64_t n_src, int C,
                       int crop_h, int crop_w, const int32_t* table, int n, int groups, int nrow, int pad, int maxres, int sep_height,
                       int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes, void* stream);

/* Explaining a score (csrc/explain.hip): the ViT tower's input gradient, its reduction to one map per image, and the map laid over
 * the pictures.  All three check their arguments before any launch (EOE_ERR_ARG, naming the argument); n == 0 returns 0 without one.
 *   eoe_unpatchify_grad  dx fp32 [n, 3, res, res] from dpatches fp32 [n (res / patch)^2, 3 patch^2] (column = c patch^2 + ky patch + kx,
 *        eoe_patchify's map): dx = dpatches * scale_inv / std[c] (std DEVICE float[3], or NULL: no Normalize was fused).  patch % 4 == 0,
 *        patch <= 1024,
 *        res % patch == 0, both buffers 16-byte aligned.  scale_inv a power of two and std NULL: a bit copy of the rearranged values.
 *   eoe_saliency_map     s fp32 [n, H, W] from g fp32 [n, C, H, W] (C 1 or 3): EOE_SALIENCY_MAX max_c |g_c| (exact), EOE_SALIENCY_L2
 *        sqrt(sum_c g_c^2), EOE_SALIENCY_GRADXINPUT sum_c |g_c x_c| (x of g's shape; NULL otherwise).  pool > 1: every aligned pool x pool
 *        block carries the mean of its pixels (pool must divide H and W).  No atomics: the same bytes on every run.
 *   eoe_heat_overlay_u8  out uint8 [n, H, W, 3] (a form eoe_grid_u8 takes) from s fp32 [n, H, W] and the pictures -- pictures_u8 == 0: fp32
 *        NCHW in ToTensor's scale (img = 255 x); else uint8 NHWC -- with C 1 or 3 (one channel fills the three).  Per image lo / hi are
 *        the minimum / maximum of the finite entries of s, t = (s - lo) / (hi - lo), t = 0 where hi == lo, where no entry is finite and
 *        at a non-finite entry;  byte_c = clamp(floor(img_c (1 - alpha t) + col_c alpha t + 0.5), 0, 255), col = (255, 0, 0), alpha in
 *        [0, 1]; fp32 operations in this order, no contraction.  One launch, the reduction in a fixed order. */
enum { EOE_SALIENCY_MAX = 0, EOE_SALIENCY_L2 = 1, EOE_SALIENCY_GRADXINPUT = 2 };
int eoe_unpatchify_grad(const float* dpatches, const float* std, float scale_inv, float* dx, int n, int res, int patch, void* stream);
int eoe_saliency_map(const float* g, const float* x, float* s, int n, int C, int H, int W, int mode, int pool, void* stream);
int eoe_heat_overlay_u8(const float* s, const void* pictures, int pictures_u8, uint8_t* out, int n, int C, int H, int W, float alpha,
                        void* stream);

/* The last hop of a BatchNorm CNN's input gradient (csrc/explain.hip): a first-layer convolution's data gradient, back to the image.
 *   dx[i, c, hi, wi] = (scale_inv / std[c]) * sum over (co, ky, kx) of dy[(i, ho, wo), co] * w[co, c, ky, kx]
 *                      with ho * stride - pad + ky == hi and wo * stride - pad + kx == wi
 * dy [n Ho Wo, cout] as the BatchNorm backward leaves it, 16-bit or fp32 by `dtype` (EOE_F16 | EOE_BF16 | EOE_F32), aligned to four of
 * its elements; w the fp32 parameter [cout, cin, kh, kw] as it is; dx fp32 NCHW [n, cin, Hi, Wi]; std DEVICE float[cin] of a fused
 * Normalize (NULL: none); scale_inv undoes the gradient scale.  Ho = (Hi + 2 pad - kh) / stride + 1, likewise Wo.  Served: cin 1 or 3,
 * cout % 4 == 0 (at most 4096), kh == kw odd and at most 7, stride 1 or 2, 0 <= pad < kh, images up to 2048 x 2048 and no smaller than the
 * kernel once padded; anything else is EOE_ERR_ARG before any launch; n == 0 returns 0 without one.  One launch, no patch matrix, no
 * atomics: every element is an fp32 fmaf chain over (co, ky, kx) in that order on the fp32 weights, the same bits on every run; a pixel
 * no tap reaches is 0. */
int eoe_conv_image_dgrad(const void* dy, const float* w, const float* std, float scale_inv, float* dx, int n, int cin, int cout, int Hi,
                         int Wi, int kh, int kw, int stride, int pad, int dtype, void* stream);

/* Attention rollout (csrc/rollout.hip; Abnar & Zuidema 2020): where a ViT tower's class token attends, from the forward pass alone.  All
 * three check their arguments before any launch (EOE_ERR_ARG: a null pointer, n, L or heads <= 0, L > EOE_ATTN_LONG_MAX_L, an unknown dtype or
 * fuse code, residual outside [0, 1), r_out overlapping r_in or probs, L != grid^2 + 1), allocate nothing, use no atomics and give the same
 * bits on every run.
 *   eoe_attn_probs    probs fp32 [n, L, L] from qkv in eoe_attn_fwd's layout (16-bit [n*L, 3*D], q | k | v, D = heads*64; the V third is never
 *        read), 1 <= L <= EOE_ATTN_LONG_MAX_L: per head P_h = softmax_rows(q_h k_h^T / 8) -- the products on the matrix cores with fp32
 *        accumulation, the softmax in fp32 with the row maximum subtracted -- fused over the heads: EOE_FUSE_MEAN the sum over h = 0 ..
 *        heads - 1 in that order times 1.0f / heads, EOE_FUSE_MAX / EOE_FUSE_MIN the element-wise maximum / minimum.
 *   eoe_rollout_step  r_out = A^ r_in per image, fp32 [n, L, L] each: A^ = (1 - residual) probs + residual I with every row divided by its own
 *        fp32 sum (a row whose sum is 0 or not finite is the identity row; a sum within 2^-20 of one -- its own worst-case rounding -- is
 *        taken as one, so an already normalised row keeps its bits); A^ is formed on the fly.  r_in == NULL is the identity (r_out =
 *        A^), bit for bit what an explicit identity gives; with residual == 0 and rows that sum to one that is probs itself.
 *   eoe_rollout_map   maps fp32 [n, grid*patch, grid*patch] from r fp32 [n, L, L], L == grid^2 + 1: pixel (y, x) = r[i, 0, 1 + (y / patch) *
 *        grid + x / patch] -- the class token's row without the class column, every patch block constant (a form eoe_heat_overlay_u8 takes). */
enum { EOE_FUSE_MEAN = 0, EOE_FUSE_MAX = 1, EOE_FUSE_MIN = 2 };
int eoe_attn_probs(const void* qkv, float* probs, int n, int L, int heads, int dtype, int fuse, void* stream);
int eoe_rollout_step(const float* probs, const float* r_in, float* r_out, int n, int L, float residual, void* stream);
int eoe_rollout_map(const float* r, float* maps, int n, int L, int grid, int patch, void* stream);

/* Grad-CAM (csrc/gradcam.hip; Selvaraju et al. 2017) for the WideResNet + CBAM encoder: A = a layer's activation, dA = the gradient of the
 * score at it, both fp32 NHWC [n, h, w, C], C % 4 == 0, h, w >= 1, 16-byte aligned, fewer than 2^31 elements.  All three check their
 * arguments before any launch (EOE_ERR_ARG: a null pointer, C % 4, a misaligned pointer, 2^31 elements or more, H < h or W < w, an
 * unknown mode); n == 0 returns 0 without one.  No atomics, every sum in an order that depends on the shape alone: the same bytes on
 * every run.  fp32 operations without contraction.
 *   eoe_cam_weights   alpha fp32 [n, C] = (1 / hw) sum_p dA[i, p, c]
 *   eoe_cam_map       map fp32 [n, h, w]: EOE_CAM_GRADCAM relu(sum_c alpha[i, c] A[i, p, c]) (dA may be NULL), EOE_CAM_HIRESCAM
 *        relu(sum_c dA[i, p, c] A[i, p, c]) (alpha may be NULL: no weights launch is needed).  relu keeps a NaN.
 *   eoe_cam_upsample  out fp32 [n, H, W] from map fp32 [n, h, w], bilinear at the positions of interpolate(align_corners=False): source
 *        index max((dst + 0.5) h / H - 0.5, 0), split exactly (in integers) into its integer part i0 and its fraction l1, the
 *        neighbour i1 = min(i0 + 1, h - 1); out = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11), l0 = 1 - l1.  Any h <= H <= 32768
 *        and w <= W <= 32768, integer ratio or not; h == w == 1 gives a constant map, h == H and w == W a bit copy. */
enum { EOE_CAM_GRADCAM = 0, EOE_CAM_HIRESCAM = 1 };
int eoe_cam_weights(const float* dA, float* alpha, int n, int h, int w, int C, void* stream);
int eoe_cam_map(const float* A, const float* dA, const float* alpha, float* map, int n, int h, int w, int C, int mode, void* stream);
int eoe_cam_upsample(const float* map, float* out, int n, int h, int w, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * in-library kernel timing (used by bench.py for the roofline line): while enabled, every entry point brackets
 * its kernel launches with hipEvents on the stream it launches on and records the algorithmic flops / bytes.
 * eoe_prof_collect synchronises the recorded events and aggregates them per kernel name.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct {
    char name[32];
    int64_t launches;
    double total_ms;   /* sum of per-launch durations */
    double flops;      /* sum of algorithmic floating-point operations (2 per MAC) */
    double bytes;      /* sum of algorithmic HBM bytes (inputs read once + outputs written once) */
} eoe_prof_entry;
int eoe_prof_enable(int on);

/* Box calibration probes (bench.py prints them in its line so that numbers from different boxes can be compared; not on the product path):
 * a bare v_mfma_f32_16x16x32_f16 loop -- `blocks` workgroups of 4 waves, 8 independent accumulators each, `iters` rounds of 8 MFMAs per wave
 * (2 * 16*16*32 * 8 * iters * 4 * blocks FLOP), out: blocks * 256 floats or NULL -- and a 16-byte-per-lane streaming copy. */
int eoe_probe_mfma_f16(float* out, int iters, int blocks, void* stream);
int eoe_probe_copy(void* dst, const void* src, int64_t bytes, void* stream);

/* tuning switches for A/B measurements inside one process ("nt_flags": see gemm.hip) */
int eoe_set_option(const char* name, int value);
int eoe_get_option(const char* name, int* value);    /* the current value (callers that change a switch restore what they found) */
/* "nt_last_kernel" (read-only diagnostics, like "tn256_launches"): the route the last eoe_gemm_nt of this process took, set on the host by the
 * launcher; tests assert it so that a case which falls through to another kernel fails instead of passing.
 * "nt_last_form" (read-only, set with it): mi * 16 + ni of that route -- rows per tile / 32 of the two-workgroup and one-wave kernels, columns
 * per tile / 32 of the persistent kernel; it tells the kernels behind EOE_NT_KERNEL_GATHER apart (0: the 256 x 64 kernel) */
enum {
    EOE_NT_KERNEL_NONE = 0,                  /* no NT GEMM launched yet */
    EOE_NT_KERNEL_PERSISTENT_256x128 = 1,    /* gemm.hip: eight waves, one workgroup per CU, 256 x 128 tiles */
    EOE_NT_KERNEL_PERSISTENT_256x96 = 2,     /*           the same with 256 x 96 tiles */
    EOE_NT_KERNEL_NARROW_256x64 = 3,         /*           N <= 64: 256 x 64 tiles, two workgroups per CU */
    EOE_NT_KERNEL_PERSISTENT_NARROW = 4,     /*           N <= 64: the persistent kernel with 256 x 64 tiles */
    EOE_NT_KERNEL_TWO_WG_128 = 5,            /*           two workgroups per CU, 128 x 128 tiles */
    EOE_NT_KERNEL_TWO_WG_160 = 6,            /*           two workgroups per CU, 160 x 128 tiles */
    EOE_NT_KERNEL_WIDE_160x256x32 = 7,       /*           two workgroups per CU, 160 x 256 tiles, 32-deep k-tiles */
    EOE_NT_KERNEL_ONE_WAVE_160x256 = 8,      /* gemm256.hip: one wave per SIMD, 160 x 256 tiles */
    EOE_NT_KERNEL_ONE_WAVE_256x256 = 9,      /*              one wave per SIMD, 256 x 256 tiles */
    EOE_NT_KERNEL_EIGHT_WAVE = 10,           /* gemm_w8.hip: eight waves, 256 x 256 tiles, data-parallel */
    EOE_NT_KERNEL_EIGHT_WAVE_STREAM_K = 11,  /*              its stream-K form */
    EOE_NT_KERNEL_SPLIT_K = 12,              /* gemm.hip: split k (eoe_gemm_args.split_k) + the in-order finish kernel */
    EOE_NT_KERNEL_GATHER = 13                /* any implicit-convolution (gather != 0) form */
};
/* The route eoe_gemm_nt would take with these arguments and the current "nt_flags" on a device of `ncu` CUs (ncu <= 0: the current device's
 * count), in *kernel; nothing is launched and "nt_last_kernel" stays.  The same argument checks as eoe_gemm_nt.  With ncu > 0 the call touches
 * no GPU and reads nothing behind the operand pointers: any non-null, 16-byte aligned addresses will do, on a machine without a GPU too. */
int eoe_gemm_nt_route(const eoe_gemm_args* args, int ncu, int* kernel);
/* diagnostics only (EOE_GEMM_STAMP=1): in-kernel s_memtime stamps of the last eoe_gemm_nt launch, 16 words per workgroup */
int eoe_debug_gemm_stamps(unsigned long long* out, int n_words);
int eoe_prof_collect(eoe_prof_entry* out, int max_entries, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* EOE_HIP_H */
