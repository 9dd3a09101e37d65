// Multi-scale modes (MSM): the label-conditioned input filters of the reference's frequency-analysis experiments
// (`utils/transformations.py`: GpuDFTLowPassFilter :294-323, GpuDFTHighPassFilter :228-255, Blur :141-153, MinMaxNorm
// :177-185), applied to fp32 NCHW batches in the [0, 1] pixel scale, before Normalize.
//
// lpf / hpf.  The reference runs fft2 -> fftshift -> mask -> ifftshift -> ifft2 -> .real -> MinMaxNorm.  Both masks are
// separable (lpf: m (x) m) or one minus a separable box (hpf: 1 - b (x) b), so with the 1-D operator G = F^-1 S^-1 diag(mask) S F
// (n x n, complex; S = fftshift) the filters are exact operator products on the real image X:
//   lpf  Y = Re(A X A^T)          A built from the kept band m
//   hpf  Y = X - Re(B X B^T)      B built from the zeroed central band b
// G is a projection onto a contiguous set of DFT frequencies, G = c I + s U U^H with U = the n x r matrix of those frequency
// columns / sqrt(n): either the kept set (c = 0, s = 1) or its complement (c = 1, s = -1), whichever is smaller, r <= n / 2.
//   * n <= 32 (CIFAR 32^2, CNN28 28^2): one workgroup per image, the whole image and the dense G in LDS, one launch with the
//     MinMax fused; fp64 accumulation of fp32 operands.
//   * larger n (224^2): the rank-limited form as batched GEMMs (fp32 operands and intermediates, fp64 accumulation) through a
//     caller workspace.  With Ut = [Re U | Im U]
//     (n x 2r, real), A1 = Ut^T X, A2 = X Ut, T = A1 Ut and M = [[Trr - Tii, Tri + Tir], [Tir + Tri, Tii - Trr]]:
//       Re(G X G^T) = c^2 X + cs (Ut A1 + A2 Ut^T) + s^2 Ut M Ut^T
//     i.e. 10 r n^2 multiply-adds per plane instead of the dense form's 4 n^3.  A final pass (one workgroup per image) applies
//     MinMaxNorm and copies the unselected rows.
// A fully zeroed spectrum (lpf with e = n/2 at even n, hpf with e = n/2 at even n) gives exact zeros and 0/0 = NaN rows, as the
// reference does.  magnitude <= 0 is the identity: a bit-exact copy, no MinMax.
//
// blur.  kornia's gaussian_blur2d(img, (k, k), (sigma, sigma)) with reflect borders: separable, normalised exp(-x^2 / 2 sigma^2)
// taps, x = arange(k) - k // 2, k = max(min(2*int(sigma/2) + 1, 2*(W//2) - 1), 3); two passes through the workspace.  The taps
// travel in the kernel arguments, at most BLUR_MAX_TAPS = 223 of them: every k of the rule for images up to 224 wide, in
// 892 bytes of taps (the whole argument block stays under 1 KiB).
//
// Row selection: rows[i] != 0 filters image i, rows[i] == 0 copies it bit for bit; rows == NULL filters every image.  The op
// is out of place (y must not alias x).
#include "common.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int SMALL_N = 32;          // largest side of the one-workgroup LDS path
constexpr int SMALL_C = 3;
constexpr int BLUR_MAX_TAPS = 223;   // k at W = 224 and sigma >= 222 (the ImageNet driver's 256)

struct BlurTaps { float w[BLUR_MAX_TAPS]; };

__device__ __forceinline__ bool selected(const uint8_t* rows, int img) { return rows == nullptr || rows[img] != 0; }

// workgroup min / max of one value per thread (256 threads)
__device__ void block_minmax(float& mn, float& mx, float* red) {
    const int t = threadIdx.x;
    red[t] = mn; red[256 + t] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { red[t] = fminf(red[t], red[t + s]); red[256 + t] = fmaxf(red[256 + t], red[256 + t + s]); }
        __syncthreads();
    }
    mn = red[0]; mx = red[256];
    __syncthreads();
}

// ---- n <= 32: one workgroup per image ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void msm_small_kernel(const float* __restrict__ x, float* __restrict__ y, const uint8_t* __restrict__ rows,
                                                        const float* __restrict__ oper, int C, int n, float alpha, float beta) {
    __shared__ float X[SMALL_C * SMALL_N * SMALL_N];
    __shared__ float Gr[SMALL_N * SMALL_N], Gi[SMALL_N * SMALL_N];
    __shared__ float Tr[SMALL_N * SMALL_N], Ti[SMALL_N * SMALL_N];
    __shared__ float red[512];
    const int b = blockIdx.x, t = threadIdx.x, nn = n * n, tot = C * nn;
    const float* xb = x + (size_t)b * tot;
    float* yb = y + (size_t)b * tot;
    if (!selected(rows, b)) {
        for (int i = t; i < tot; i += 256) yb[i] = xb[i];
        return;
    }
    for (int i = t; i < tot; i += 256) X[i] = xb[i];
    for (int i = t; i < nn; i += 256) { Gr[i] = oper[i]; Gi[i] = oper[nn + i]; }
    __syncthreads();
    for (int c = 0; c < C; ++c) {
        float* Xc = X + c * nn;
        for (int e = t; e < nn; e += 256) {                    // T = X G^T
            const int i = e / n, j = e % n;
            double ar = 0.0, ai = 0.0;
            for (int l = 0; l < n; ++l) {
                const double v = Xc[i * n + l];
                ar += v * Gr[j * n + l];
                ai += v * Gi[j * n + l];
            }
            Tr[e] = (float)ar; Ti[e] = (float)ai;
        }
        __syncthreads();
        for (int e = t; e < nn; e += 256) {                    // Y = alpha X + beta (Gr Tr - Gi Ti)
            const int i = e / n, j = e % n;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += (double)Gr[i * n + k] * Tr[k * n + j] - (double)Gi[i * n + k] * Ti[k * n + j];
            Xc[e] = (float)((double)alpha * Xc[e] + (double)beta * acc);
        }
        __syncthreads();
    }
    float mn = INFINITY, mx = -INFINITY;
    for (int i = t; i < tot; i += 256) { mn = fminf(mn, X[i]); mx = fmaxf(mx, X[i]); }
    block_minmax(mn, mx, red);
    const float d = mx - mn;                                    // = max(y - min) (rounding is monotonic)
    for (int i = t; i < tot; i += 256) yb[i] = (X[i] - mn) / d;
}

// ---- batched GEMM for the rank-limited form: fp32 operands, fp64 accumulation --------------------------------------------
// C[p] = ax * Xin[p] + ab * A[p] B[p] (+ C[p] when accumulate), A: M x K (lda), B: K x N (ldb), row-major; a stride of 0 shares
// the operand between planes.  Plane p belongs to image p / C; planes of unselected images are skipped.  The sums run in fp64
// and the epilogue rounds once to fp32, as msm_small_kernel does: when U holds the DC column (lpf on its kept set, magnitude
// >= 56 at 224^2), A1 and T carry the plane's column and total sums (T's DC entry is n / 2 for a mean-0.5 image, against
// outputs of order 1), and fp32 sums put lpf 64 / 100 at about 4x the reference's own fp32 distance from fp64.
struct GemmB {
    const float* A; const float* B; float* Cm; const float* Xin;
    long long sA, sB, sC, sX;
    int M, N, K, lda, ldb, ldc, ldx;
    float ax, ab;
    int accumulate, C;
    const uint8_t* rows;
};

__global__ __launch_bounds__(256) void msm_gemm_kernel(GemmB g) {
    __shared__ float As[16][64 + 4];
    __shared__ float Bs[16][64 + 4];
    const int p = blockIdx.z;
    if (!selected(g.rows, p / g.C)) return;
    const float* A = g.A + p * g.sA;
    const float* B = g.B + p * g.sB;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < g.K; k0 += 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + q * 256;                        // 1024 elements of each tile
            const int am = e / 16, ak = e % 16;               // A tile 64 x 16
            const int gm = m0 + am, gk = k0 + ak;
            As[ak][am] = (gm < g.M && gk < g.K) ? A[(size_t)gm * g.lda + gk] : 0.f;
            const int bk = e / 64, bn = e % 64;               // B tile 16 x 64
            const int gk2 = k0 + bk, gn = n0 + bn;
            Bs[bk][bn] = (gk2 < g.K && gn < g.N) ? B[(size_t)gk2 * g.ldb + gn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double a[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty * 4 + i]; bv[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    float* Cm = g.Cm + p * g.sC;
    const float* X = g.Xin ? g.Xin + p * g.sX : nullptr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty * 4 + i;
        if (gm >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx * 4 + j;
            if (gn >= g.N) continue;
            double v = (double)g.ab * acc[i][j];
            if (X) v += (double)g.ax * X[(size_t)gm * g.ldx + gn];
            float* dst = Cm + (size_t)gm * g.ldc + gn;
            if (g.accumulate) v += *dst;
            *dst = (float)v;
        }
    }
}

// M = [[Trr - Tii, Tri + Tir], [Tir + Tri, Tii - Trr]] per plane (T and M: 2r x 2r)
__global__ __launch_bounds__(256) void msm_core_kernel(const float* __restrict__ T, float* __restrict__ Mo, int r, int planes, int C,
                                                       const uint8_t* __restrict__ rows) {
    const int w = 2 * r, per = w * w;
    const size_t total = (size_t)planes * per;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(e / per), q = (int)(e % per), a = q / w, b = q % w;
        if (!selected(rows, p / C)) continue;
        const float* Tp = T + (size_t)p * per;
        const int a2 = a < r ? a + r : a - r, b2 = b < r ? b + r : b - r;     // partner block index
        const float v = (a < r) == (b < r) ? Tp[q] - Tp[a2 * w + b2]     // rr: Trr - Tii; ii: Tii - Trr
                                           : Tp[q] + Tp[a2 * w + b2];    // ri: Tri + Tir; ir: Tir + Tri
        Mo[(size_t)p * per + q] = v;
    }
}

// final pass, one workgroup per image: MinMaxNorm of the filtered rows (in place in y), bit copy of the unselected ones
__global__ __launch_bounds__(256) void msm_minmax_kernel(const float* __restrict__ x, float* __restrict__ y, const uint8_t* __restrict__ rows,
                                                         long long per_img) {
    __shared__ float red[512];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* xb = x + (size_t)b * per_img;
    float* yb = y + (size_t)b * per_img;
    if (!selected(rows, b)) {
        for (long long i = t; i < per_img; i += 256) yb[i] = xb[i];
        return;
    }
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = t; i < per_img; i += 256) { const float v = yb[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    block_minmax(mn, mx, red);
    const float d = mx - mn;
    for (long long i = t; i < per_img; i += 256) yb[i] = (yb[i] - mn) / d;
}

// ---- blur ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(256) void blur_h_kernel(const float* __restrict__ x, float* __restrict__ tmp, const uint8_t* __restrict__ rows,
                                                     int n_img, int C, int H, int W, int k, BlurTaps taps) {
    const size_t per = (size_t)C * H * W, total = (size_t)n_img * per;
    const int h = k / 2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        if (!selected(rows, (int)(e / per))) continue;
        const int j = (int)(e % W);
        const float* row = x + (e - j);
        float acc = 0.f;
        for (int q = 0; q < k; ++q) acc = fmaf(taps.w[q], row[reflect(j + q - h, W)], acc);
        tmp[e] = acc;
    }
}

__global__ __launch_bounds__(256) void blur_v_kernel(const float* __restrict__ x, const float* __restrict__ tmp, float* __restrict__ y,
                                                     const uint8_t* __restrict__ rows, int n_img, int C, int H, int W, int k, BlurTaps taps) {
    const size_t per = (size_t)C * H * W, total = (size_t)n_img * per;
    const int h = k / 2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        if (!selected(rows, (int)(e / per))) { y[e] = x[e]; continue; }
        const int j = (int)(e % W), i = (int)((e / W) % H);
        const float* col = tmp + (e - (size_t)i * W);          // (plane, row 0, column j)
        float acc = 0.f;
        for (int q = 0; q < k; ++q) acc = fmaf(taps.w[q], col[(size_t)reflect(i + q - h, H) * W], acc);
        y[e] = acc;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int clipped_e(int n, int magnitude) { return magnitude < n / 2 ? magnitude : n / 2; }

// the unshifted frequencies the 1-D operator G keeps (lpf: shifted band [e, n - e); hpf: the zeroed central band
// [n//2 - e, n//2 + e), which B projects onto); shifted index i holds frequency (i - n//2) mod n
std::vector<int> kept_freqs(int op, int n, int e) {
    std::vector<int> f;
    for (int i = 0; i < n; ++i) {
        const bool keep = op == EOE_MSM_LPF ? (i >= e && i < n - e) : (i >= n / 2 - e && i < n / 2 + e);
        if (keep) f.push_back(((i - n / 2) % n + n) % n);
    }
    return f;
}

int blur_taps(int magnitude, int W, int* k_out, BlurTaps* taps) {
    const double sigma = (double)magnitude;
    int k = 2 * (int)(sigma / 2.0) + 1;                     // Blur.__init__: 2 * int(int(sigma / 2) + 0.5) + 1
    const int cap = 2 * (W / 2) - 1;
    if (k > cap) k = cap;
    if (k < 3) k = 3;
    *k_out = k;
    if (k > BLUR_MAX_TAPS) return eoe_set_error(EOE_ERR_UNSUPPORTED, "msm_filter: blur with %d taps (at most %d)", k, BLUR_MAX_TAPS);
    if (taps) {
        double w[BLUR_MAX_TAPS], s = 0.0;
        for (int q = 0; q < k; ++q) { const double xx = q - k / 2; w[q] = exp(-xx * xx / (2.0 * sigma * sigma)); s += w[q]; }
        for (int q = 0; q < BLUR_MAX_TAPS; ++q) taps->w[q] = q < k ? (float)(w[q] / s) : 0.f;
    }
    return 0;
}

}  // namespace

extern "C" int eoe_msm_operator(int op, int n, int magnitude, int rank_limited, double* re, double* im, int* cols_out, double* cs_out) {
    EOE_CHECK_ARG((op == EOE_MSM_LPF || op == EOE_MSM_HPF) && n >= 2 && n <= 4096 && (rank_limited == 0 || rank_limited == 1),
                  "msm_operator: op must be EOE_MSM_LPF / EOE_MSM_HPF, 2 <= n <= 4096, rank_limited 0 or 1");
    const int e = magnitude <= 0 ? 0 : clipped_e(n, magnitude);
    std::vector<int> f;
    if (magnitude <= 0) {                                  // identity
        for (int i = 0; i < n; ++i) f.push_back(i);
    } else {
        f = kept_freqs(op, n, e);
    }
    const int kept = (int)f.size();
    double c = 0.0, s = 1.0;
    if (rank_limited && kept > n - kept) {                 // the complement is smaller: G = I - U_c U_c^H
        std::vector<bool> in(n, false);
        for (int v : f) in[v] = true;
        f.clear();
        for (int v = 0; v < n; ++v) if (!in[v]) f.push_back(v);
        c = 1.0; s = -1.0;
    }
    const int cols = rank_limited ? (int)f.size() : n;
    if (cols_out) *cols_out = cols;
    if (cs_out) { cs_out[0] = rank_limited ? c : 0.0; cs_out[1] = rank_limited ? s : 1.0; }
    if (!re || !im) return 0;                              // size query
    const double two_pi = 6.283185307179586476925286766559;
    if (rank_limited) {                                    // U[j][t] = exp(2 pi i f_t j / n) / sqrt(n)
        const double inv = 1.0 / sqrt((double)n);
        for (int j = 0; j < n; ++j)
            for (int t = 0; t < cols; ++t) {
                const long long ph = ((long long)f[t] * j) % n;
                re[(size_t)j * cols + t] = cos(two_pi * ph / n) * inv;
                im[(size_t)j * cols + t] = sin(two_pi * ph / n) * inv;
            }
        return 0;
    }
    // dense G[j][k] = (1/n) sum_f exp(2 pi i f (j - k) / n); exact identity / zero for the full / empty set
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) {
            double ar = 0.0, ai = 0.0;
            if (kept == n) {
                ar = j == k ? 1.0 : 0.0;
            } else {
                for (int v : f) {
                    const long long ph = (((long long)v * (j - k)) % n + n) % n;
                    ar += cos(two_pi * ph / n);
                    ai += sin(two_pi * ph / n);
                }
                ar /= n; ai /= n;
            }
            re[(size_t)j * n + k] = ar;
            im[(size_t)j * n + k] = ai;
        }
    return 0;
}

extern "C" int eoe_msm_workspace(int op, int n_img, int C, int H, int W, int magnitude, int* form_out, size_t* bytes_out) {
    EOE_CHECK_ARG(form_out && bytes_out && n_img > 0 && C > 0 && H > 0 && W > 0, "msm_workspace: bad args");
    EOE_CHECK_ARG(op == EOE_MSM_LPF || op == EOE_MSM_HPF || op == EOE_MSM_BLUR, "msm_workspace: unknown op %d", op);
    *form_out = EOE_MSM_FORM_NONE;
    *bytes_out = 0;
    if (magnitude <= 0) return 0;
    if (op == EOE_MSM_BLUR) {
        int k = 0;
        if (int rc = blur_taps(magnitude, W, &k, nullptr)) return rc;
        EOE_CHECK_ARG(k / 2 < H && k / 2 < W, "msm_workspace: blur with %d taps on %d x %d", k, H, W);
        *bytes_out = sizeof(float) * (size_t)n_img * C * H * W;
        return 0;
    }
    EOE_CHECK_ARG(H == W, "msm_workspace: lpf / hpf need square images (%d x %d)", H, W);
    if (H <= SMALL_N) {
        EOE_CHECK_ARG(C <= SMALL_C, "msm_workspace: at most %d channels", SMALL_C);
        *form_out = EOE_MSM_FORM_DENSE;
        return 0;
    }
    int r = 0;
    if (int rc = eoe_msm_operator(op, H, magnitude, 1, nullptr, nullptr, &r, nullptr)) return rc;
    *form_out = EOE_MSM_FORM_RANK;
    const size_t n = (size_t)H;
    *bytes_out = sizeof(float) * (size_t)n_img * C * (6 * (size_t)r * n + 8 * (size_t)r * r);
    return 0;
}

extern "C" int eoe_msm_filter(int op, const float* x, float* y, const uint8_t* rows, int n_img, int C, int H, int W, int magnitude,
                              const float* oper, void* workspace, size_t workspace_bytes, void* stream) {
    EOE_CHECK_ARG(x && y && x != y, "msm_filter: null or aliased x / y (the op is out of place)");
    int form = 0;
    size_t need = 0;
    if (int rc = eoe_msm_workspace(op, n_img, C, H, W, magnitude, &form, &need)) return rc;
    EOE_CHECK_ARG(workspace_bytes >= need && (need == 0 || workspace), "msm_filter: workspace of %zu bytes, %zu needed",
                  workspace_bytes, need);
    EOE_CHECK_ARG(form == EOE_MSM_FORM_NONE || oper, "msm_filter: null operator");
    EOE_CHECK_ARG((long long)n_img * C <= 65535, "msm_filter: at most 65535 planes per call");
    hipStream_t st = (hipStream_t)stream;
    const size_t per = (size_t)C * H * W, total = (size_t)n_img * per;
    if (magnitude <= 0) {                                  // identity: bit copy
        ProfScope ps("msm_copy", 0, 8.0 * total, stream);
        if (hipMemcpyAsync(y, x, sizeof(float) * total, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return eoe_set_error(EOE_ERR_LAUNCH, "msm_filter: copy failed");
        return 0;
    }
    if (op == EOE_MSM_BLUR) {
        BlurTaps taps;
        int k = 0;
        if (int rc = blur_taps(magnitude, W, &k, &taps)) return rc;
        ProfScope ps("msm_blur", 4.0 * k * total, 16.0 * total, stream);
        float* tmp = (float*)workspace;
        size_t g = (total + 255) / 256;
        if (g > 16384) g = 16384;
        hipLaunchKernelGGL(blur_h_kernel, dim3((unsigned)g), dim3(256), 0, st, x, tmp, rows, n_img, C, H, W, k, taps);
        EOE_CHECK_LAUNCH("msm_blur_h");
        hipLaunchKernelGGL(blur_v_kernel, dim3((unsigned)g), dim3(256), 0, st, x, tmp, y, rows, n_img, C, H, W, k, taps);
        EOE_CHECK_LAUNCH("msm_blur_v");
        return 0;
    }
    const float alpha = op == EOE_MSM_LPF ? 0.f : 1.f, beta = op == EOE_MSM_LPF ? 1.f : -1.f;
    const int n = H;
    if (form == EOE_MSM_FORM_DENSE) {
        ProfScope ps("msm_small", 8.0 * n * n * n * (double)C * n_img, 8.0 * total, stream);
        hipLaunchKernelGGL(msm_small_kernel, dim3((unsigned)n_img), dim3(256), 0, st, x, y, rows, oper, C, n, alpha, beta);
        EOE_CHECK_LAUNCH("msm_small");
        return 0;
    }
    int r = 0;
    double cs[2] = {0.0, 1.0};
    if (int rc = eoe_msm_operator(op, n, magnitude, 1, nullptr, nullptr, &r, cs)) return rc;
    const int w = 2 * r, planes = n_img * C;
    const long long nn = (long long)n * n;
    const float* Ut = oper;                                // n x 2r
    const float* UtT = oper + (size_t)n * w;               // 2r x n
    float* A1 = (float*)workspace;                         // per plane 2r x n
    float* A2 = A1 + (size_t)planes * w * n;               // n x 2r
    float* T = A2 + (size_t)planes * n * w;                // 2r x 2r
    float* Mm = T + (size_t)planes * w * w;                // 2r x 2r
    float* L = Mm + (size_t)planes * w * w;                // n x 2r
    const float c = (float)cs[0], s = (float)cs[1];
    ProfScope ps("msm_rank", 20.0 * r * nn * planes, 12.0 * total, stream);
    auto gemm = [&](const float* A, long long sA, int lda, const float* B, long long sB, int ldb, float* Cm, long long sC, int ldc,
                    int M, int N, int K, float ab, const float* X, long long sX, int ldx, float ax, int accumulate) -> int {
        GemmB g{A, B, Cm, X, sA, sB, sC, sX, M, N, K, lda, ldb, ldc, ldx, ax, ab, accumulate, C, rows};
        dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64), (unsigned)planes);
        hipLaunchKernelGGL(msm_gemm_kernel, grid, dim3(256), 0, st, g);
        EOE_CHECK_LAUNCH("msm_gemm");
        return 0;
    };
    int rc = 0;
    if (r > 0) {
        rc |= gemm(UtT, 0, n, x, nn, n, A1, (long long)w * n, n, w, n, n, 1.f, nullptr, 0, 0, 0.f, 0);           // A1 = Ut^T X
        rc |= gemm(x, nn, n, Ut, 0, w, A2, (long long)n * w, w, n, w, n, 1.f, nullptr, 0, 0, 0.f, 0);            // A2 = X Ut
        rc |= gemm(A1, (long long)w * n, n, Ut, 0, w, T, (long long)w * w, w, w, w, n, 1.f, nullptr, 0, 0, 0.f, 0);  // T = A1 Ut
        size_t g = ((size_t)planes * w * w + 255) / 256;
        if (g > 16384) g = 16384;
        hipLaunchKernelGGL(msm_core_kernel, dim3((unsigned)g), dim3(256), 0, st, T, Mm, r, planes, C, rows);
        EOE_CHECK_LAUNCH("msm_core");
        // L = beta s^2 Ut M + beta c s A2
        rc |= gemm(Ut, 0, w, Mm, (long long)w * w, w, L, (long long)n * w, w, n, w, w, beta * s * s, A2, (long long)n * w, w,
                   beta * c * s, 0);
    }
    // Y = (alpha + beta c^2) X + beta c s Ut A1  (K = 0 when r = 0: Y = (alpha + beta c^2) X)
    rc |= gemm(Ut, 0, w, A1, (long long)w * n, n, y, nn, n, n, n, w, beta * c * s, x, nn, n, alpha + beta * c * c, 0);
    if (r > 0) rc |= gemm(L, (long long)n * w, w, UtT, 0, n, y, nn, n, n, n, w, 1.f, nullptr, 0, 0, 0.f, 1);   // Y += L Ut^T
    if (rc) return rc;
    hipLaunchKernelGGL(msm_minmax_kernel, dim3((unsigned)n_img), dim3(256), 0, st, x, y, rows, (long long)per);
    EOE_CHECK_LAUNCH("msm_minmax");
    return 0;
}
