// Explaining an anomaly score: where in the image it comes from.  Three streaming kernels over n x C x H x W elements, next to grid.hip:
//   eoe_unpatchify_grad  the last hop of the ViT tower's input gradient: dpatches fp32 [n g^2, 3 p^2] (dtok x conv1.weight, an NT GEMM) back to
//                        pixels, dx fp32 [n, 3, res, res].  The inverse of patchify_kernel's index map (column = c p^2 + ky p + kx), times
//                        1 / std[c] where a Normalize was fused into the forward, times scale_inv (undoes the fp16 gradient scale: a power of
//                        two, so exactly).  One thread per 16 bytes of dx; p % 4 == 0 keeps a quad inside one patch row, so the read is 16
//                        bytes too, and p / 4 neighbouring lanes read one contiguous patch row.
//   eoe_saliency_map     the C-channel gradient reduced to one map per image: max_c |g_c|, sqrt(sum_c g_c^2) or sum_c |g_c x_c|; with pool = p
//                        every aligned p x p block carries its mean (the patch-level map of a ViT).  One wavefront per block: lanes sum their
//                        pixels in index order, a xor-shuffle tree adds the lanes -- no atomics, the same bytes on every run.
//   eoe_heat_overlay_u8  the map laid over the pictures: per image t = (s - min) / (max - min) over the finite entries (0 for a constant map
//                        and for a non-finite entry), byte = floor(img (1 - alpha t) + col alpha t + 0.5), col = (255, 0, 0), uint8 NHWC out: a
//                        form eoe_grid_u8 takes.  One workgroup per image, so the min / max reduction and the colouring are one launch and the
//                        reduction order is fixed.
// Compiled without floating-point contraction: explain.saliency_np / overlay_np state the same fp32 operations one by one.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EX_NT = 256;
constexpr int OV_NT = 1024;

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }      // false for NaN as well

// ------------------------------------------------------------------------------------------ unpatchify
// quad q of dx in [img][c][y][x / 4] order
__global__ __launch_bounds__(EX_NT) void unpatchify_grad_kernel(const float* __restrict__ dp, const float* __restrict__ stdv,
                                                                float scale_inv, float* __restrict__ dx, unsigned total, int res, int p,
                                                                FDiv rq_d, FDiv res_d, FDiv p_d) {
    const unsigned q = blockIdx.x * EX_NT + threadIdx.x;
    if (q >= total) return;
    unsigned row, xq, ic, y, img, c, py, ky, px, kx;
    rq_d.divmod(q, row, xq);
    res_d.divmod(row, ic, y);
    img = ic / 3u, c = ic - img * 3u;
    p_d.divmod(y, py, ky);
    p_d.divmod(xq * 4u, px, kx);
    const unsigned g = (unsigned)(res / p);
    const size_t src = ((size_t)(img * g + py) * g + px) * ((size_t)3 * p * p) + (size_t)c * p * p + ky * p + kx;
    f32x4 v = *reinterpret_cast<const f32x4*>(dp + src);
    const float m = stdv ? scale_inv * (1.0f / stdv[c]) : scale_inv;
    v[0] *= m, v[1] *= m, v[2] *= m, v[3] *= m;
    *reinterpret_cast<f32x4*>(dx + (size_t)q * 4) = v;
}

// ------------------------------------------------------------------------------------------ saliency
enum { SAL_MAX = EOE_SALIENCY_MAX, SAL_L2 = EOE_SALIENCY_L2, SAL_GXI = EOE_SALIENCY_GRADXINPUT };

__device__ __forceinline__ float sal_value(const float* g, const float* x, int C, int mode) {
    if (mode == SAL_MAX) return C == 1 ? fabsf(g[0]) : fmaxf(fmaxf(fabsf(g[0]), fabsf(g[1])), fabsf(g[2]));
    if (mode == SAL_L2) return C == 1 ? sqrtf(g[0] * g[0]) : sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    return C == 1 ? fabsf(g[0] * x[0]) : fabsf(g[0] * x[0]) + fabsf(g[1] * x[1]) + fabsf(g[2] * x[2]);
}

// the values of pixels [off, off + (VEC ? 4 : 1)) of image `img` (off within the plane)
template <bool VEC>
__device__ __forceinline__ void sal_load(const float* __restrict__ g, const float* __restrict__ x, size_t img, size_t off, int C, size_t plane,
                                         int mode, float* out) {
    constexpr int K = VEC ? 4 : 1;
    float gv[3][K], xv[3][K];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= C) break;
        const size_t at = (img * C + c) * plane + off;
        if (VEC) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(g + at);
            const f32x4 b = mode == SAL_GXI ? *reinterpret_cast<const f32x4*>(x + at) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K; ++k) gv[c][k] = a[k], xv[c][k] = b[k];
        } else {
            gv[c][0] = g[at];
            xv[c][0] = mode == SAL_GXI ? x[at] : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float gg[3] = {gv[0][k], C == 3 ? gv[1][k] : 0.f, C == 3 ? gv[2][k] : 0.f};
        const float xx[3] = {xv[0][k], C == 3 ? xv[1][k] : 0.f, C == 3 ? xv[2][k] : 0.f};
        out[k] = sal_value(gg, xx, C, mode);
    }
}

// no pooling: element e of the flattened [n][plane / K] maps (VEC: plane % 4 == 0)
template <bool VEC>
__global__ __launch_bounds__(EX_NT) void saliency_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ s,
                                                         unsigned total, int C, int plane, int mode, FDiv per_d) {
    constexpr int K = VEC ? 4 : 1;
    const unsigned e = blockIdx.x * EX_NT + threadIdx.x;
    if (e >= total) return;
    unsigned img, r;
    per_d.divmod(e, img, r);
    float v[K];
    sal_load<VEC>(g, x, img, (size_t)r * K, C, (size_t)plane, mode, v);
    float* o = s + (size_t)img * plane + (size_t)r * K;
    if (VEC) *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[VEC ? 1 : 0], v[VEC ? 2 : 0], v[VEC ? 3 : 0]};
    else o[0] = v[0];
}

// pooling: wavefront wb of the launch owns block (img, by, bx); its pieces are the block's pixels (VEC: quads) in row-major order
template <bool VEC>
__global__ __launch_bounds__(EX_NT) void saliency_pool_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ s,
                                                              unsigned nblocks, int C, int H, int W, int mode, int p, FDiv bw_d, FDiv bh_d,
                                                              FDiv pk_d) {
    constexpr int K = VEC ? 4 : 1;
    const unsigned wb = blockIdx.x * (EX_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wb >= nblocks) return;                          // whole wavefronts leave: the shuffles below see all 64 lanes
    unsigned t, bx, img, by;
    bw_d.divmod(wb, t, bx);
    bh_d.divmod(t, img, by);
    const unsigned pieces = (unsigned)(p * p) / K;
    const size_t plane = (size_t)H * W, origin = (size_t)by * p * W + (size_t)bx * p;
    float acc = 0.f;
    for (unsigned e = lane; e < pieces; e += 64) {
        unsigned yy, xk;
        pk_d.divmod(e, yy, xk);
        float v[K];
        sal_load<VEC>(g, x, img, origin + (size_t)yy * W + xk * K, C, plane, mode, v);
#pragma unroll
        for (int k = 0; k < K; ++k) acc += v[k];
    }
    const float mean = wave_sum(acc) / (float)(p * p);
    for (unsigned e = lane; e < pieces; e += 64) {
        unsigned yy, xk;
        pk_d.divmod(e, yy, xk);
        float* o = s + (size_t)img * plane + origin + (size_t)yy * W + xk * K;
        if (VEC) *reinterpret_cast<f32x4*>(o) = f32x4{mean, mean, mean, mean};
        else o[0] = mean;
    }
}

// ------------------------------------------------------------------------------------------ overlay
// one workgroup per image.  vec: plane % 4 == 0 and every base 16- (floats) / 4-byte (bytes) aligned
template <bool U8>
__global__ __launch_bounds__(OV_NT) void heat_overlay_kernel(const float* __restrict__ s, const void* __restrict__ pics, uint8_t* __restrict__ out,
                                                             int C, int plane, float alpha, int vec) {
    __shared__ float red[2 * (OV_NT / 64)];
    const int t = threadIdx.x;
    const size_t img = blockIdx.x;
    const float* sm = s + img * plane;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = t; i < plane; i += OV_NT) {
        const float v = sm[i];
        if (finite_f(v)) lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((t & 63) == 0) red[2 * (t >> 6)] = lo, red[2 * (t >> 6) + 1] = hi;
    __syncthreads();
    lo = red[0], hi = red[1];
#pragma unroll
    for (int w = 1; w < OV_NT / 64; ++w) lo = fminf(lo, red[2 * w]), hi = fmaxf(hi, red[2 * w + 1]);
    const float d = hi - lo;                            // no finite entry: -inf - inf = -inf, not > 0
    const bool live = d > 0.0f && finite_f(d);
    const float* pf = static_cast<const float*>(pics) + img * C * plane;
    const uint8_t* pu = static_cast<const uint8_t*>(pics) + img * plane * C;
    uint8_t* po = out + img * plane * 3;
    const int quads = (plane + 3) >> 2;
    for (int q = t; q < quads; q += OV_NT) {
        const int j0 = q * 4, cnt = min(4, plane - j0);
        const bool full = vec && cnt == 4;
        float sv[4] = {0.f, 0.f, 0.f, 0.f}, pc[3][4] = {};
        if (full) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(sm + j0);
            sv[0] = a[0], sv[1] = a[1], sv[2] = a[2], sv[3] = a[3];
        } else {
            for (int k = 0; k < cnt; ++k) sv[k] = sm[j0 + k];
        }
        if (U8) {
            if (full) {
                unsigned wds[3];
                for (int w = 0; w < C; ++w) wds[w] = reinterpret_cast<const unsigned*>(pu + (size_t)j0 * C)[w];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int b = C == 3 ? k * 3 + c : k;
                        pc[c][k] = (float)((wds[b >> 2] >> (8 * (b & 3))) & 255u);
                    }
            } else {
                for (int k = 0; k < cnt; ++k)
                    for (int c = 0; c < 3; ++c) pc[c][k] = (float)pu[(size_t)(j0 + k) * C + (C == 3 ? c : 0)];
            }
        } else {
            for (int c = 0; c < 3; ++c) {
                const float* pl = pf + (size_t)(C == 3 ? c : 0) * plane + j0;
                if (full) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(pl);
                    pc[c][0] = a[0] * 255.0f, pc[c][1] = a[1] * 255.0f, pc[c][2] = a[2] * 255.0f, pc[c][3] = a[3] * 255.0f;
                } else {
                    for (int k = 0; k < cnt; ++k) pc[c][k] = pl[k] * 255.0f;
                }
            }
        }
        unsigned bytes[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float tt = (live && finite_f(sv[k])) ? (sv[k] - lo) / d : 0.0f;
            const float a = alpha * tt, ia = 1.0f - a;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float col = c == 0 ? 255.0f : 0.0f;
                const float r = floorf(pc[c][k] * ia + col * a + 0.5f);
                bytes[k * 3 + c] = k < cnt ? (unsigned)(int)fminf(fmaxf(r, 0.0f), 255.0f) : 0u;
            }
        }
        if (full) {
            unsigned* ow = reinterpret_cast<unsigned*>(po + (size_t)j0 * 3);
#pragma unroll
            for (int w = 0; w < 3; ++w)
                ow[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | (bytes[4 * w + 3] << 24);
        } else {
            for (int b = 0; b < cnt * 3; ++b) po[(size_t)j0 * 3 + b] = (uint8_t)bytes[b];
        }
    }
}

// ------------------------------------------------------------------------------------------ first-layer dgrad
// One workgroup per (image, 16 x 16 tile of dx), one thread per pixel, all CIN channels of it in registers.  The output channels of dy go
// through LDS CD_CC at a time: the tile's window of dy (every position a tap of the tile reaches, at most 22 x 22) transposed to
// [channel][position] fp32 -- so the lanes of a wave, which sit side by side in the tile, read side by side -- and the weights of those
// channels as [channel][tap][4] (CIN == 1: [channel][tap]), one LDS read per tap.  A pixel sums its taps in the fixed order (channel,
// ky, kx) with fmaf: no atomics, the same bits on every run.  With stride 2 a pixel has taps only at ky = (hi + pad) % 2 + 2 j (and
// likewise kx): the tap loops step by the stride from that start.
constexpr int CD_T = 16;                       // tile edge
constexpr int CD_CC = 16;                      // channels of dy per round
constexpr int CD_MAXK = 7;                     // largest kernel edge
constexpr int CD_DT = CD_T + CD_MAXK - 1;      // 22: the widest window (stride 1, 7 x 7)
// plane stride of the transposed window: >= CD_DT^2 = 484 and = 2 (mod 8), so that the four planes a lane quad writes (4 channels apart, 8
// positions per 32 lanes) fall on 32 different banks
constexpr int CD_PS = 490;
static_assert(CD_PS >= CD_DT * CD_DT && CD_PS % 8 == 2, "plane stride of the dy window");

template <typename T> __device__ __forceinline__ void cd_load4(const T* p, float* o) { unpack4<T>(*reinterpret_cast<const u32x2*>(p), o); }
template <> __device__ __forceinline__ void cd_load4<float>(const float* p, float* o) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
}

// K, S: kernel edge and stride as compile-time constants (0: the run-time values k_rt, s_rt)
template <typename T, int CIN, int K, int S>
__global__ __launch_bounds__(CD_T* CD_T) void conv_image_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                                      const float* __restrict__ stdv, float scale_inv, float* __restrict__ dx,
                                                                      int cout, int Hi, int Wi, int Ho, int Wo, int k_rt, int s_rt, int pad,
                                                                      int tiles_x) {
    constexpr int WS = CIN == 1 ? 1 : 4;
    constexpr int MAXJ = K ? (K + (S ? S : 1) - 1) / (S ? S : 1) : CD_MAXK;
    __shared__ float dyl[CD_CC * CD_PS];
    __shared__ __attribute__((aligned(16))) float wl[CD_CC * CD_MAXK * CD_MAXK * WS];
    const int k = K ? K : k_rt, s = S ? S : s_rt, kk = k * k;
    const int t = threadIdx.x, ty = t >> 4, tx = t & (CD_T - 1);
    const int img = blockIdx.x, tyb = (int)blockIdx.y / tiles_x, txb = (int)blockIdx.y - tyb * tiles_x;
    const int hi0 = tyb * CD_T, wi0 = txb * CD_T;
    // the window of dy the tile's taps reach: rows ho with hi0 <= ho s - pad + ky < hi0 + CD_T for some ky, clipped to dy
    const int ra = hi0 + pad - (k - 1), ca = wi0 + pad - (k - 1);
    const int ho_lo = ra > 0 ? (ra + s - 1) / s : 0, wo_lo = ca > 0 ? (ca + s - 1) / s : 0;
    const int ho_hi = min(Ho - 1, (min(hi0 + CD_T, Hi) - 1 + pad) / s), wo_hi = min(Wo - 1, (min(wi0 + CD_T, Wi) - 1 + pad) / s);
    const int th = max(ho_hi - ho_lo + 1, 0), tw = max(wo_hi - wo_lo + 1, 0), npos = th * tw;      // th, tw <= CD_DT
    const unsigned tw_m = tw ? (65536u + tw - 1) / tw : 0u;      // pos / tw = pos * tw_m >> 16 for pos < 512, tw <= 22

    // the thread's taps: LDS offsets of the rows / columns of dy they read, and of their weights
    const int hi = hi0 + ty, wi = wi0 + tx;
    const bool live = hi < Hi && wi < Wi;
    const int ky0 = (hi + pad) % s, kx0 = (wi + pad) % s;
    int roff[MAXJ], coff[MAXJ], wyo[MAXJ], wxo[MAXJ];
    bool rok[MAXJ], cok[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int ky = ky0 + j * s, kx = kx0 + j * s;
        const int a = hi + pad - ky, b = wi + pad - kx;          // multiples of s
        const int ho = a / s, wo = b / s;
        rok[j] = live && ky < k && a >= 0 && ho < Ho;
        cok[j] = live && kx < k && b >= 0 && wo < Wo;
        roff[j] = rok[j] ? (ho - ho_lo) * tw : 0;
        coff[j] = cok[j] ? wo - wo_lo : 0;
        wyo[j] = ky < k ? ky * k * WS : 0;
        wxo[j] = kx < k ? kx * WS : 0;
    }

    float acc[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
    for (int co0 = 0; co0 < cout; co0 += CD_CC) {
        const int cc = min(CD_CC, cout - co0);                   // a multiple of 4
        __syncthreads();                                         // the round before has been read
        for (int e = t; e < npos * (CD_CC / 4); e += CD_T * CD_T) {
            const int pos = e >> 2, q = (e & 3) * 4;
            if (q >= cc) continue;
            const int r = (int)(((unsigned)pos * tw_m) >> 16), c = pos - r * tw;
            float v[4];
            cd_load4<T>(dy + (((size_t)img * Ho + ho_lo + r) * Wo + wo_lo + c) * cout + co0 + q, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) dyl[(q + i) * CD_PS + pos] = v[i];
        }
        const float* wsrc = w + (size_t)co0 * CIN * kk;           // the round's weights: cc * CIN * kk contiguous floats
        for (int e = t; e < cc * CIN * kk; e += CD_T * CD_T) {
            const int col = e / (CIN * kk), rem = e - col * (CIN * kk), c = rem / kk, tap = rem - c * kk;
            wl[(col * kk + tap) * WS + c] = wsrc[e];
        }
        __syncthreads();
        for (int col = 0; col < cc; ++col) {
            const float* dp = dyl + col * CD_PS;
            const float* wp = wl + col * kk * WS;
#pragma unroll
            for (int jy = 0; jy < MAXJ; ++jy) {
                if (jy * s >= k) break;                           // the same in every lane
#pragma unroll
                for (int jx = 0; jx < MAXJ; ++jx) {
                    if (jx * s >= k) break;
                    const float d = (rok[jy] && cok[jx]) ? dp[roff[jy] + coff[jx]] : 0.f;
                    const float* wt = wp + wyo[jy] + wxo[jx];
                    if (CIN == 1) {
                        acc[0] = fmaf(d, wt[0], acc[0]);
                    } else {
                        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wt);      // the 4th entry is never written nor used
#pragma unroll
                        for (int c = 0; c < CIN; ++c) acc[c] = fmaf(d, w4[c], acc[c]);
                    }
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
        const float m = stdv ? scale_inv * (1.0f / stdv[c]) : scale_inv;
        dx[(((size_t)img * CIN + c) * Hi + hi) * Wi + wi] = acc[c] * m;
    }
}

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <typename T>
void conv_image_dgrad_launch(const void* dy, const float* w, const float* stdv, float scale_inv, float* dx, int n, int cin, int cout, int Hi,
                             int Wi, int Ho, int Wo, int k, int stride, int pad, hipStream_t st) {
    const int tiles_x = (Wi + CD_T - 1) / CD_T, tiles_y = (Hi + CD_T - 1) / CD_T;
    const dim3 grid((unsigned)n, (unsigned)(tiles_x * tiles_y)), block(CD_T * CD_T);
    const T* d = static_cast<const T*>(dy);
#define EOE_CD(CIN, K, S) \
    hipLaunchKernelGGL((conv_image_dgrad_kernel<T, CIN, K, S>), grid, block, 0, st, d, w, stdv, scale_inv, dx, cout, Hi, Wi, Ho, Wo, k, stride, pad, tiles_x)
    const bool five = k == 5 && stride == 1;                    // CNN32's and CNN28's first layer
    if (cin == 1) { if (five) EOE_CD(1, 5, 1); else EOE_CD(1, 0, 0); }
    else { if (five) EOE_CD(3, 5, 1); else EOE_CD(3, 0, 0); }
#undef EOE_CD
}

}  // namespace

extern "C" int eoe_conv_image_dgrad(const void* dy, const float* w, const float* stdv, float scale_inv, float* dx, int n, int cin, int cout,
                                    int Hi, int Wi, int kh, int kw, int stride, int pad, int dtype, void* stream) {
    EOE_CHECK_ARG(dy && w && dx, "conv_image_dgrad: null dy, w or dx");
    EOE_CHECK_ARG(n >= 0, "conv_image_dgrad: n must not be negative, not %d", n);
    EOE_CHECK_ARG(cin == 1 || cin == 3, "conv_image_dgrad: cin must be 1 or 3, not %d", cin);
    EOE_CHECK_ARG(cout >= 4 && cout % 4 == 0 && cout <= 4096, "conv_image_dgrad: cout %% 4 != 0 or outside [4, 4096] (cout = %d)", cout);
    EOE_CHECK_ARG(kh == kw && kh >= 1 && kh <= CD_MAXK && kh % 2 == 1, "conv_image_dgrad: the kernel must be square, odd and at most 7, not %d x %d",
                  kh, kw);
    EOE_CHECK_ARG(stride == 1 || stride == 2, "conv_image_dgrad: stride must be 1 or 2, not %d", stride);
    EOE_CHECK_ARG(pad >= 0 && pad < kh, "conv_image_dgrad: pad must be in [0, kh), not %d", pad);
    EOE_CHECK_ARG(Hi >= 1 && Wi >= 1 && Hi <= 2048 && Wi <= 2048, "conv_image_dgrad: images of %d x %d (at most 2048 x 2048)", Hi, Wi);
    EOE_CHECK_ARG(Hi + 2 * pad >= kh && Wi + 2 * pad >= kw, "conv_image_dgrad: the padded %d x %d image is smaller than the kernel", Hi, Wi);
    EOE_CHECK_ARG(dtype == EOE_F16 || dtype == EOE_BF16 || dtype == EOE_F32, "conv_image_dgrad: dtype %d is none of EOE_F16, EOE_BF16, EOE_F32",
                  dtype);
    EOE_CHECK_ARG(scale_inv == scale_inv && fabsf(scale_inv) < INFINITY, "conv_image_dgrad: scale_inv must be finite");
    EOE_CHECK_ARG(aligned(dy, dtype == EOE_F32 ? 16 : 8) && aligned(w, 4) && aligned(dx, 4) && (!stdv || aligned(stdv, 4)),
                  "conv_image_dgrad: dy must be aligned to four of its elements, w, dx and std to 4 bytes");
    const int Ho = (Hi + 2 * pad - kh) / stride + 1, Wo = (Wi + 2 * pad - kw) / stride + 1;
    const long long dy_elems = (long long)n * Ho * Wo * cout, dx_elems = (long long)n * cin * Hi * Wi;
    EOE_CHECK_ARG(dy_elems < (1ll << 31) && dx_elems < (1ll << 31), "conv_image_dgrad: %lld elements of dy or %lld of dx exceed 32-bit indexing",
                  dy_elems, dx_elems);
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("conv_image_dgrad", 2.0 * (double)dy_elems * cin * kh * kw,
                 (double)dy_elems * (dtype == EOE_F32 ? 4.0 : 2.0) + 4.0 * (double)dx_elems + 4.0 * (double)cout * cin * kh * kw, stream);
    if (dtype == EOE_F16) conv_image_dgrad_launch<f16_t>(dy, w, stdv, scale_inv, dx, n, cin, cout, Hi, Wi, Ho, Wo, kh, stride, pad, st);
    else if (dtype == EOE_BF16) conv_image_dgrad_launch<bf16_t>(dy, w, stdv, scale_inv, dx, n, cin, cout, Hi, Wi, Ho, Wo, kh, stride, pad, st);
    else conv_image_dgrad_launch<float>(dy, w, stdv, scale_inv, dx, n, cin, cout, Hi, Wi, Ho, Wo, kh, stride, pad, st);
    EOE_CHECK_LAUNCH("conv_image_dgrad");
    return 0;
}

extern "C" int eoe_unpatchify_grad(const float* dpatches, const float* stdv, float scale_inv, float* dx, int n, int res, int patch,
                                   void* stream) {
    EOE_CHECK_ARG(dpatches && dx, "unpatchify_grad: null dpatches or dx");
    EOE_CHECK_ARG(n >= 0, "unpatchify_grad: n must not be negative, not %d", n);
    EOE_CHECK_ARG(patch >= 4 && patch % 4 == 0, "unpatchify_grad: patch %% 4 != 0 (patch = %d)", patch);
    EOE_CHECK_ARG(patch <= 1024, "unpatchify_grad: patch must be at most 1024, not %d", patch);
    EOE_CHECK_ARG(res >= patch && res <= 32768 && res % patch == 0, "unpatchify_grad: res %% patch != 0 (res = %d, patch = %d)", res, patch);
    EOE_CHECK_ARG(scale_inv == scale_inv && fabsf(scale_inv) < INFINITY, "unpatchify_grad: scale_inv must be finite");
    EOE_CHECK_ARG(aligned(dpatches, 16) && aligned(dx, 16) && (!stdv || aligned(stdv, 4)), "unpatchify_grad: dpatches and dx must be 16-byte aligned");
    const long long quads = (long long)n * 3 * res * (res / 4);
    EOE_CHECK_ARG(quads < (1ll << 31), "unpatchify_grad: n * 3 * res^2 / 4 = %lld quads exceed 32-bit indexing", quads);
    if (n == 0) return 0;
    ProfScope ps("unpatchify_grad", 4.0 * (double)quads, 32.0 * (double)quads, stream);
    hipLaunchKernelGGL(unpatchify_grad_kernel, dim3((unsigned)((quads + EX_NT - 1) / EX_NT)), dim3(EX_NT), 0, (hipStream_t)stream, dpatches, stdv,
                       scale_inv, dx, (unsigned)quads, res, patch, FDiv((unsigned)(res / 4)), FDiv((unsigned)res), FDiv((unsigned)patch));
    EOE_CHECK_LAUNCH("unpatchify_grad");
    return 0;
}

extern "C" int eoe_saliency_map(const float* g, const float* x, float* s, int n, int C, int H, int W, int mode, int pool, void* stream) {
    EOE_CHECK_ARG(g && s, "saliency_map: null g or s");
    EOE_CHECK_ARG(mode == SAL_MAX || mode == SAL_L2 || mode == SAL_GXI, "saliency_map: mode %d is none of EOE_SALIENCY_*", mode);
    EOE_CHECK_ARG(mode != SAL_GXI || x, "saliency_map: gradxinput needs x");
    EOE_CHECK_ARG(C == 1 || C == 3, "saliency_map: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(n >= 0 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "saliency_map: n = %d maps of %d x %d", n, H, W);
    EOE_CHECK_ARG(pool >= 0 && pool <= 4096, "saliency_map: pool must be in [0, 4096], not %d", pool);
    EOE_CHECK_ARG(pool <= 1 || (H % pool == 0 && W % pool == 0), "saliency_map: pool = %d does not divide H = %d and W = %d", pool, H, W);
    EOE_CHECK_ARG(aligned(g, 4) && aligned(s, 4) && (!x || aligned(x, 4)), "saliency_map: g, x and s must be 4-byte aligned");
    const long long plane = (long long)H * W, total = (long long)n * C * plane;
    EOE_CHECK_ARG(total < (1ll << 31), "saliency_map: n * C * H * W = %lld elements exceed 32-bit indexing", total);
    if (n == 0) return 0;
    const bool a16 = aligned(g, 16) && aligned(s, 16) && (mode != SAL_GXI || aligned(x, 16));
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("saliency_map", 6.0 * (double)total, 4.0 * ((double)total * (mode == SAL_GXI ? 2 : 1) + (double)n * plane), stream);
    if (pool <= 1) {
        const bool vec = a16 && plane % 4 == 0;
        const unsigned per = (unsigned)(vec ? plane / 4 : plane), cnt = per * (unsigned)n;
        const dim3 grid((cnt + EX_NT - 1) / EX_NT);
        if (vec) hipLaunchKernelGGL(saliency_kernel<true>, grid, dim3(EX_NT), 0, st, g, x, s, cnt, C, (int)plane, mode, FDiv(per));
        else hipLaunchKernelGGL(saliency_kernel<false>, grid, dim3(EX_NT), 0, st, g, x, s, cnt, C, (int)plane, mode, FDiv(per));
    } else {
        const bool vec = a16 && pool % 4 == 0;                      // then W % 4 == 0 as well: every quad of a block is 16-byte aligned
        const unsigned bw = (unsigned)(W / pool), bh = (unsigned)(H / pool), nb = bw * bh * (unsigned)n;
        const dim3 grid((nb + EX_NT / 64 - 1) / (EX_NT / 64));
        if (vec) hipLaunchKernelGGL(saliency_pool_kernel<true>, grid, dim3(EX_NT), 0, st, g, x, s, nb, C, H, W, mode, pool, FDiv(bw), FDiv(bh),
                                    FDiv((unsigned)(pool / 4)));
        else hipLaunchKernelGGL(saliency_pool_kernel<false>, grid, dim3(EX_NT), 0, st, g, x, s, nb, C, H, W, mode, pool, FDiv(bw), FDiv(bh),
                                FDiv((unsigned)pool));
    }
    EOE_CHECK_LAUNCH("saliency_map");
    return 0;
}

extern "C" int eoe_heat_overlay_u8(const float* s, const void* pictures, int pictures_u8, uint8_t* out, int n, int C, int H, int W, float alpha,
                                   void* stream) {
    EOE_CHECK_ARG(s && pictures && out, "heat_overlay_u8: null s, pictures or out");
    EOE_CHECK_ARG(C == 1 || C == 3, "heat_overlay_u8: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(alpha >= 0.0f && alpha <= 1.0f, "heat_overlay_u8: alpha must be in [0, 1], not %g", (double)alpha);
    EOE_CHECK_ARG(n >= 0 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "heat_overlay_u8: n = %d maps of %d x %d", n, H, W);
    EOE_CHECK_ARG(aligned(s, 4) && (pictures_u8 || aligned(pictures, 4)), "heat_overlay_u8: s and fp32 pictures must be 4-byte aligned");
    const long long plane = (long long)H * W, total = (long long)n * 3 * plane;
    EOE_CHECK_ARG(total < (1ll << 31), "heat_overlay_u8: n * 3 * H * W = %lld bytes exceed 32-bit indexing", total);
    if (n == 0) return 0;
    const int vec = plane % 4 == 0 && aligned(s, 16) && aligned(out, 4) && aligned(pictures, pictures_u8 ? 4 : 16);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("heat_overlay_u8", 12.0 * (double)n * plane, (double)n * plane * (8.0 + 3.0 + (pictures_u8 ? 1.0 : 4.0) * C), stream);
    if (pictures_u8) hipLaunchKernelGGL(heat_overlay_kernel<true>, dim3((unsigned)n), dim3(OV_NT), 0, st, s, pictures, out, C, (int)plane, alpha, vec);
    else hipLaunchKernelGGL(heat_overlay_kernel<false>, dim3((unsigned)n), dim3(OV_NT), 0, st, s, pictures, out, C, (int)plane, alpha, vec);
    EOE_CHECK_LAUNCH("heat_overlay_u8");
    return 0;
}
