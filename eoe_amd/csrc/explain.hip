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

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

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
