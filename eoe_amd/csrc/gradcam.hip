// Grad-CAM (Selvaraju et al. 2017) and HiResCAM maps for the WideResNet + CBAM encoder: a late layer's activation A and the gradient dA of
// the score at it, both fp32 NHWC [n, h, w, C], turned into one map per image.  Three streaming kernels, next to explain.hip:
//   eoe_cam_weights   alpha[i, c] = (1 / hw) sum_p dA[i, p, c].  One workgroup per (image, group of at most 256 channels): a thread owns four
//                     channels (one 16-byte load per pixel) and every rpb-th pixel, rpb = 256 / (channel quads of the group); it adds its
//                     pixels in index order, the rpb partial sums are added through LDS in row order.  The order depends on (hw, C) alone.
//   eoe_cam_map       map[i, p] = relu(sum_c alpha[i, c] A[i, p, c]) (EOE_CAM_GRADCAM) or relu(sum_c dA[i, p, c] A[i, p, c]) (EOE_CAM_HIRESCAM).
//                     lpp = the largest power of two <= min(16, C / 4) lanes per pixel: lane s adds the channels 4 s + 4 lpp k + r in the
//                     order (k, r), a xor-shuffle tree adds the lanes.  The order depends on C alone.
//   eoe_cam_upsample  bilinear [n, h, w] -> [n, H, W] at the positions of interpolate(align_corners=False): source index
//                     max(((2 dst + 1) h - H) / (2 H), 0), its integer part and its fraction taken in integer arithmetic (the fraction is one
//                     fp32 division of two exact integers), value = l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11) with l0 = 1 - l1.
// No atomics anywhere: the same bytes on every run.  relu keeps a NaN (v > 0 || v != v ? v : 0).  Compiled without floating-point
// contraction: every product and every sum is rounded once, which is what the error bound of the tests counts.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CAM_NT = 256;

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ float relu_keep_nan(float v) { return (v > 0.f || v != v) ? v : 0.f; }

// grid (n, channel groups); cpb = channel quads per group (a divisor of 256), rpb = 256 / cpb pixel rows per step
__global__ __launch_bounds__(CAM_NT) void cam_weights_kernel(const float* __restrict__ dA, float* __restrict__ alpha, int HW, int C, int cpb) {
    __shared__ f32x4 ls[CAM_NT];
    const int img = blockIdx.x, rpb = CAM_NT / cpb;
    const int tc = threadIdx.x % cpb, rl = threadIdx.x / cpb;
    const int q = blockIdx.y * cpb + tc;                       // channel quad
    const bool live = q * 4 < C;
    const float* base = dA + (size_t)img * HW * C + (size_t)(live ? q : 0) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = 8;
    int p = rl;
    if (live) {
        for (; p + (U - 1) * rpb < HW; p += U * rpb) {
            f32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const f32x4*>(base + (size_t)(p + u * rpb) * C);
#pragma unroll
            for (int u = 0; u < U; ++u) s += v[u];
        }
        for (; p < HW; p += rpb) s += *reinterpret_cast<const f32x4*>(base + (size_t)p * C);
    }
    ls[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0 && live) {
        for (int k = 1; k < rpb; ++k) s += ls[threadIdx.x + k * cpb];
        const float hw = (float)HW;
        *reinterpret_cast<f32x4*>(alpha + (size_t)img * C + q * 4) = f32x4{s[0] / hw, s[1] / hw, s[2] / hw, s[3] / hw};
    }
}

// HIRES: the second operand is dA[i, p, c] (same layout as A); else alpha[i, c]
template <bool HIRES>
__global__ __launch_bounds__(CAM_NT) void cam_map_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ map,
                                                         unsigned P, int HW, int C, int lpp) {
    const unsigned ppb = CAM_NT / lpp, sub = threadIdx.x & (lpp - 1);
    const unsigned p = blockIdx.x * ppb + threadIdx.x / lpp;
    const bool live = p < P;                                   // dead lanes still take part in the shuffles
    float s = 0.f;
    if (live) {
        const float* a = A + (size_t)p * C;
        const float* b = HIRES ? B + (size_t)p * C : B + (size_t)(p / (unsigned)HW) * C;
        for (int c = sub * 4; c < C; c += lpp * 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(a + c);
            const f32x4 y = *reinterpret_cast<const f32x4*>(b + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += x[r] * y[r];
        }
    }
    for (int sft = lpp >> 1; sft >= 1; sft >>= 1) s += __shfl_xor(s, sft, 64);
    if (live && sub == 0) map[p] = relu_keep_nan(s);
}

// source row / column of destination index d: i0, i1 and the weight of i1
__device__ __forceinline__ void cam_src(int d, int in, int out, int& i0, int& i1, float& l1) {
    const int num = (2 * d + 1) * in - out, den = 2 * out;    // (d + 0.5) in / out - 0.5 = num / den
    if (num <= 0) { i0 = 0; l1 = 0.f; }
    else { i0 = num / den; l1 = (float)(num - i0 * den) / (float)den; }
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// one thread per K = (VEC ? 4 : 1) neighbouring outputs of a row
template <bool VEC>
__global__ __launch_bounds__(CAM_NT) void cam_upsample_kernel(const float* __restrict__ m, float* __restrict__ out, unsigned total, int h, int w,
                                                              int H, int W, FDiv wq_d, FDiv H_d) {
    constexpr int K = VEC ? 4 : 1;
    const unsigned e = blockIdx.x * CAM_NT + threadIdx.x;
    if (e >= total) return;
    unsigned row, xq, img, y;
    wq_d.divmod(e, row, xq);
    H_d.divmod(row, img, y);
    int y0, y1;
    float ly1;
    cam_src((int)y, h, H, y0, y1, ly1);
    const float ly0 = 1.f - ly1;
    const float* r0 = m + ((size_t)img * h + y0) * w;
    const float* r1 = m + ((size_t)img * h + y1) * w;
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int x0, x1;
        float lx1;
        cam_src((int)xq * K + k, w, W, x0, x1, lx1);
        const float lx0 = 1.f - lx1;
        v[k] = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
    }
    float* o = out + (size_t)row * W + (size_t)xq * K;
    if (VEC) *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[VEC ? 1 : 0], v[VEC ? 2 : 0], v[VEC ? 3 : 0]};
    else o[0] = v[0];
}

int cam_check_act(const char* who, int n, int h, int w, int C, long long* elems) {
    EOE_CHECK_ARG(n >= 0, "%s: n must not be negative, not %d", who, n);
    EOE_CHECK_ARG(h >= 1 && w >= 1, "%s: the map must be at least 1 x 1, not %d x %d", who, h, w);
    EOE_CHECK_ARG(C >= 4 && C % 4 == 0, "%s: C %% 4 != 0 or C < 4 (C = %d)", who, C);
    EOE_CHECK_ARG((long long)h * w < (1ll << 31), "%s: a map of %d x %d exceeds 32-bit indexing", who, h, w);
    *elems = (long long)n * h * w * C;
    EOE_CHECK_ARG(*elems < (1ll << 31), "%s: n * h * w * C = %lld elements exceed 32-bit indexing", who, *elems);
    return 0;
}

}  // namespace

extern "C" int eoe_cam_weights(const float* dA, float* alpha, int n, int h, int w, int C, void* stream) {
    EOE_CHECK_ARG(dA && alpha, "cam_weights: null dA or alpha");
    long long elems;
    EOE_TRY(cam_check_act("cam_weights", n, h, w, C, &elems));
    EOE_CHECK_ARG(aligned(dA, 16) && aligned(alpha, 16), "cam_weights: dA and alpha must be 16-byte aligned");
    if (n == 0) return 0;
    int cpb = 1;
    while (cpb < 64 && cpb * 4 < C) cpb *= 2;                  // the smallest power of two that covers C / 4, at most 64
    const int groups = (C / 4 + cpb - 1) / cpb;
    EOE_CHECK_ARG(groups <= 65535, "cam_weights: C = %d is too large", C);
    ProfScope ps("cam_weights", (double)elems, 4.0 * ((double)elems + (double)n * C), stream);
    hipLaunchKernelGGL(cam_weights_kernel, dim3((unsigned)n, (unsigned)groups), dim3(CAM_NT), 0, (hipStream_t)stream, dA, alpha, h * w, C, cpb);
    EOE_CHECK_LAUNCH("cam_weights");
    return 0;
}

extern "C" int eoe_cam_map(const float* A, const float* dA, const float* alpha, float* map, int n, int h, int w, int C, int mode, void* stream) {
    EOE_CHECK_ARG(A && map, "cam_map: null A or map");
    EOE_CHECK_ARG(mode == EOE_CAM_GRADCAM || mode == EOE_CAM_HIRESCAM, "cam_map: mode %d is none of EOE_CAM_*", mode);
    EOE_CHECK_ARG(mode != EOE_CAM_GRADCAM || alpha, "cam_map: EOE_CAM_GRADCAM needs alpha");
    EOE_CHECK_ARG(mode != EOE_CAM_HIRESCAM || dA, "cam_map: EOE_CAM_HIRESCAM needs dA");
    long long elems;
    EOE_TRY(cam_check_act("cam_map", n, h, w, C, &elems));
    const float* B = mode == EOE_CAM_HIRESCAM ? dA : alpha;
    EOE_CHECK_ARG(aligned(A, 16) && aligned(B, 16) && aligned(map, 4), "cam_map: A and dA / alpha must be 16-byte aligned, map 4-byte aligned");
    if (n == 0) return 0;
    int lpp = 1;
    while (lpp < 16 && lpp * 2 * 4 <= C) lpp *= 2;             // the largest power of two <= min(16, C / 4)
    const unsigned P = (unsigned)((long long)n * h * w), ppb = CAM_NT / lpp;
    const dim3 grid((P + ppb - 1) / ppb);
    ProfScope ps("cam_map", 2.0 * (double)elems, 4.0 * ((double)elems * (mode == EOE_CAM_HIRESCAM ? 2 : 1) + (double)P), stream);
    if (mode == EOE_CAM_HIRESCAM) hipLaunchKernelGGL(cam_map_kernel<true>, grid, dim3(CAM_NT), 0, (hipStream_t)stream, A, B, map, P, h * w, C, lpp);
    else hipLaunchKernelGGL(cam_map_kernel<false>, grid, dim3(CAM_NT), 0, (hipStream_t)stream, A, B, map, P, h * w, C, lpp);
    EOE_CHECK_LAUNCH("cam_map");
    return 0;
}

extern "C" int eoe_cam_upsample(const float* map, float* out, int n, int h, int w, int H, int W, void* stream) {
    EOE_CHECK_ARG(map && out, "cam_upsample: null map or out");
    EOE_CHECK_ARG(n >= 0, "cam_upsample: n must not be negative, not %d", n);
    EOE_CHECK_ARG(h >= 1 && w >= 1, "cam_upsample: the map must be at least 1 x 1, not %d x %d", h, w);
    EOE_CHECK_ARG(H >= h && W >= w, "cam_upsample: the target %d x %d is smaller than the map %d x %d (H < h or W < w)", H, W, h, w);
    EOE_CHECK_ARG(H <= 32768 && W <= 32768, "cam_upsample: the target %d x %d exceeds 32768 x 32768", H, W);
    EOE_CHECK_ARG(aligned(map, 4) && aligned(out, 4), "cam_upsample: map and out must be 4-byte aligned");
    const long long total = (long long)n * H * W;
    EOE_CHECK_ARG(total < (1ll << 31), "cam_upsample: n * H * W = %lld elements exceed 32-bit indexing", total);
    if (n == 0) return 0;
    const bool vec = W % 4 == 0 && aligned(out, 16);
    const unsigned wq = (unsigned)(vec ? W / 4 : W), cnt = wq * (unsigned)H * (unsigned)n;
    const dim3 grid((cnt + CAM_NT - 1) / CAM_NT);
    ProfScope ps("cam_upsample", 11.0 * (double)total, 4.0 * ((double)total + (double)n * h * w), stream);
    if (vec) hipLaunchKernelGGL(cam_upsample_kernel<true>, grid, dim3(CAM_NT), 0, (hipStream_t)stream, map, out, cnt, h, w, H, W, FDiv(wq), FDiv((unsigned)H));
    else hipLaunchKernelGGL(cam_upsample_kernel<false>, grid, dim3(CAM_NT), 0, (hipStream_t)stream, map, out, cnt, h, w, H, W, FDiv(wq), FDiv((unsigned)H));
    EOE_CHECK_LAUNCH("cam_upsample");
    return 0;
}
