// The sharpen multi-scale mode: Pillow's ImageFilter.UnsharpMask(radius, percent, threshold), which the reference applies to
// the uint8 PIL image between its PIL augmentations and ToTensor (`utils/transformations.py:114-123` PilUnsharpMask: radius 2,
// percent int(magnitude * 100), threshold 3).  Pillow's arithmetic is all 8-bit integer, restated here so that the output equals
// Pillow's byte for byte (tests/golden g18):
//   blur    GaussianBlur(radius) = 3 horizontal then 3 vertical box passes (libImaging/BoxBlur.c).  The box radius R comes from
//           the Gaussian radius (_gaussian_blur_radius, computed on the host in Pillow's float / double mix); with r = (int)R,
//           ww = (uint32)(2^24 / (2R + 1)) and fw = (2^24 - (2r + 1) ww) / 2, one pass along a line with replicated edges is
//             out[x] = (ww * sum_{k=-r..r} in[x + k] + fw * (in[x - r - 1] + in[x + r + 1]) + 2^23) >> 24
//           in uint32 (at most 255 * 2^24 + 2^23), each pass rounded to uint8.
//   mask    d = src - blurred; |d| > threshold ? clamp(src + d * percent / 100, 0, 255) (C integer division) : src.
// One launch per call: a workgroup holds its (image, channel) planes in LDS (two uint8 buffers, ping-pong over the six passes)
// and re-reads the source for the final mask.  Each thread runs a sliding window over SEG outputs of a line, two LDS reads per
// output.  Planes up to 128^2 go SMALL_CAP-byte workgroups of 256 threads with several planes each, larger ones (up to 256^2)
// one plane per 1024-thread workgroup with 2 x 64 KiB of LDS.
// Two layouts: uint8 NHWC (PIL images, the resident sets) and fp32 NCHW in [0, 1], quantised q = clamp(rint(x * 255)) and
// written back as q' / 255.0f (a true division: ToTensor's bits, so batches on the k / 255 grid round-trip exactly).
// Row selection as in msm.hip: rows[i] != 0 sharpens image i, rows[i] == 0 copies it bit for bit; NULL sharpens all.
// percent == 0 is the identity (a bit copy).
#include "common.h"
#include <math.h>

namespace {

constexpr int SEG = 8;                  // outputs per thread and line segment
constexpr int SMALL_CAP = 16384, SMALL_NT = 256, SMALL_PIX = 4096;   // SMALL_PIX: pixels per workgroup to aim for
constexpr int LARGE_CAP = 65536, LARGE_NT = 1024;
constexpr float MAX_RADIUS = 256.f;
constexpr int MAX_PERCENT = 1 << 20;    // d * percent stays inside int

struct BoxConsts { int r; uint32_t ww, fw; };

__device__ __forceinline__ bool selected(const uint8_t* rows, int img) { return rows == nullptr || rows[img] != 0; }

// source pixel of plane gp (= image * C + channel) as the uint8 the filter works on
__device__ __forceinline__ int load_q(const uint8_t* src, size_t gp, int pix, int C, int HW) {
    return src[((gp / C) * HW + pix) * C + gp % C];
}
__device__ __forceinline__ int load_q(const float* src, size_t gp, int pix, int, int HW) {
    return (int)rintf(fminf(fmaxf(src[gp * HW + pix] * 255.f, 0.f), 255.f));
}
__device__ __forceinline__ size_t offset(const uint8_t*, size_t gp, int pix, int C, int HW) { return ((gp / C) * HW + pix) * C + gp % C; }
__device__ __forceinline__ size_t offset(const float*, size_t gp, int pix, int, int HW) { return gp * HW + pix; }
__device__ __forceinline__ void store(uint8_t* dst, size_t o, int v) { dst[o] = (uint8_t)v; }
__device__ __forceinline__ void store(float* dst, size_t o, int v) { dst[o] = (float)v / 255.0f; }     // ToTensor

// one box pass over the np planes in `in` (plane p at p * H * W): ROWS = along rows (lines of W pixels), else along columns
template <bool ROWS, int NT>
__device__ void box_pass(const uint8_t* in, uint8_t* out, int np, int H, int W, size_t plane0, int C, const uint8_t* rows, BoxConsts k) {
    const int len = ROWS ? W : H, per_plane = ROWS ? H : W, es = ROWS ? 1 : W;
    const int nseg = (len + SEG - 1) / SEG, lines = np * per_plane, items = lines * nseg;
    for (int it = threadIdx.x; it < items; it += NT) {
        // rows: neighbouring threads take neighbouring segments of a row; columns: neighbouring columns
        const int line = ROWS ? it / nseg : it % lines, seg = ROWS ? it % nseg : it / lines;
        const int p = line / per_plane, q = line % per_plane;
        if (!selected(rows, (int)((plane0 + p) / C))) continue;
        const uint8_t* li = in + p * H * W + (ROWS ? q * W : q);
        uint8_t* lo = out + p * H * W + (ROWS ? q * W : q);
        auto at = [&](int i) -> uint32_t { return li[(i < 0 ? 0 : (i >= len ? len - 1 : i)) * es]; };
        const int x0 = seg * SEG, x1 = min(x0 + SEG, len);
        uint32_t acc = 0;
        for (int j = -k.r; j <= k.r; ++j) acc += at(x0 + j);
        uint32_t left = at(x0 - k.r - 1), right = at(x0 + k.r + 1);
        for (int x = x0; x < x1; ++x) {
            lo[x * es] = (uint8_t)((acc * k.ww + (left + right) * k.fw + (1u << 23)) >> 24);
            const uint32_t drop = at(x - k.r);                 // slide to x + 1 (uint32 wrap-around cancels)
            acc += right - drop;
            left = drop;
            right = at(x + k.r + 2);
        }
    }
}

template <typename T, int CAP, int NT>
__global__ __launch_bounds__(NT) void sharpen_kernel(const T* __restrict__ src, T* __restrict__ dst, const uint8_t* __restrict__ rows,
                                                     int n_planes, int P, int C, int H, int W, BoxConsts k, int percent, int threshold) {
    __shared__ uint8_t buf[2][CAP];
    const size_t plane0 = (size_t)blockIdx.x * P;
    const int np = min(P, n_planes - (int)plane0), HW = H * W, tot = np * HW;
    for (int e = threadIdx.x; e < tot; e += NT) buf[0][e] = (uint8_t)load_q(src, plane0 + e / HW, e % HW, C, HW);
    __syncthreads();
#pragma unroll 1
    for (int pass = 0; pass < 6; ++pass) {
        const uint8_t* in = buf[pass & 1];
        uint8_t* out = buf[(pass & 1) ^ 1];
        if (pass < 3) box_pass<true, NT>(in, out, np, H, W, plane0, C, rows, k);
        else box_pass<false, NT>(in, out, np, H, W, plane0, C, rows, k);
        __syncthreads();
    }
    const uint8_t* blurred = buf[0];                           // six passes: back in buffer 0
    for (int e = threadIdx.x; e < tot; e += NT) {
        const size_t gp = plane0 + e / HW;
        const int pix = e % HW;
        const size_t o = offset(src, gp, pix, C, HW);
        if (!selected(rows, (int)(gp / C))) { dst[o] = src[o]; continue; }
        const int s = load_q(src, gp, pix, C, HW), d = s - (int)blurred[e];
        int v = s;
        if (abs(d) > threshold) {
            v = s + d * percent / 100;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
        store(dst, o, v);
    }
}

// Pillow's _gaussian_blur_radius (passes = 3) and ImagingHorizontalBoxBlur's constants, in Pillow's own float / double / uint32 mix
BoxConsts box_consts(float radius) {
#pragma clang fp contract(off)
    const float sigma2 = radius * radius / 3;
    const float L = (float)sqrt(12.0 * sigma2 + 1.0);
    const float l = (float)floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float R = l + a;
    BoxConsts k;
    k.r = (int)R;
    k.ww = (uint32_t)((uint32_t)(1 << 24) / (R * 2 + 1));
    k.fw = ((1 << 24) - (uint32_t)(k.r * 2 + 1) * k.ww) / 2;
    return k;
}

int check_args(const void* x, const void* y, int n_img, int C, int H, int W, float radius, int percent, const char* who) {
    EOE_CHECK_ARG(x && y && x != y, "%s: null or aliased input / output (the op is out of place)", who);
    EOE_CHECK_ARG(n_img > 0 && H > 0 && W > 0, "%s: n_img, H and W must be positive", who);
    EOE_CHECK_ARG(C == 1 || C == 3, "%s: C must be 1 or 3, not %d", who, C);
    EOE_CHECK_ARG(radius >= 0.f && radius <= MAX_RADIUS, "%s: radius must be in [0, %g]", who, (double)MAX_RADIUS);
    EOE_CHECK_ARG(percent >= 0 && percent <= MAX_PERCENT, "%s: percent must be in [0, %d], not %d", who, MAX_PERCENT, percent);
    EOE_CHECK_ARG((long long)H * W <= LARGE_CAP, "%s: planes of at most %d pixels (%d x %d)", who, LARGE_CAP, H, W);
    EOE_CHECK_ARG((long long)n_img * C < (1ll << 31), "%s: too many planes", who);
    return 0;
}

template <typename T>
int launch(const T* x, T* y, const uint8_t* rows, int n_img, int C, int H, int W, float radius, int percent, int threshold, void* stream,
           const char* who) {
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)n_img * C * H * W;
    if (percent == 0) {                                        // the identity: bit copy
        ProfScope ps("msm_sharpen_copy", 0, 2.0 * sizeof(T) * total, stream);
        if (hipMemcpyAsync(y, x, sizeof(T) * total, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return eoe_set_error(EOE_ERR_LAUNCH, "%s: copy failed", who);
        return 0;
    }
    const BoxConsts k = box_consts(radius);
    const int HW = H * W, n_planes = n_img * C;
    ProfScope ps(who, 6.0 * (2 * k.r + 4) * total, 2.0 * sizeof(T) * total, stream);
    if (HW <= SMALL_CAP) {
        int P = SMALL_PIX / HW;
        P = P < 1 ? 1 : (P > SMALL_CAP / HW ? SMALL_CAP / HW : P);
        const unsigned g = (unsigned)((n_planes + P - 1) / P);
        hipLaunchKernelGGL((sharpen_kernel<T, SMALL_CAP, SMALL_NT>), dim3(g), dim3(SMALL_NT), 0, st, x, y, rows, n_planes, P, C, H, W, k,
                           percent, threshold);
    } else {
        hipLaunchKernelGGL((sharpen_kernel<T, LARGE_CAP, LARGE_NT>), dim3((unsigned)n_planes), dim3(LARGE_NT), 0, st, x, y, rows, n_planes,
                           1, C, H, W, k, percent, threshold);
    }
    EOE_CHECK_LAUNCH(who);
    return 0;
}

}  // namespace

extern "C" int eoe_msm_sharpen_u8(const uint8_t* src, uint8_t* dst, const uint8_t* rows, int n_img, int H, int W, int C, float radius,
                                  int percent, int threshold, void* stream) {
    EOE_TRY(check_args(src, dst, n_img, C, H, W, radius, percent, "msm_sharpen_u8"));
    return launch(src, dst, rows, n_img, C, H, W, radius, percent, threshold, stream, "msm_sharpen_u8");
}

extern "C" int eoe_msm_sharpen_f32(const float* x, float* y, const uint8_t* rows, int n_img, int C, int H, int W, float radius,
                                   int percent, int threshold, void* stream) {
    EOE_TRY(check_args(x, y, n_img, C, H, W, radius, percent, "msm_sharpen_f32"));
    return launch(x, y, rows, n_img, C, H, W, radius, percent, threshold, stream, "msm_sharpen_f32");
}
