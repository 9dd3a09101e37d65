// On-device input pipeline: the train-time transform chain of the reference's runners
//   RandomHorizontalFlip -> RandomCrop(S, padding) -> ToTensor -> x + 0.001 * randn -> Normalize   (`main/train_cifar.py:31-38`)
//   RandomCrop(224) -> RandomHorizontalFlip -> ToTensor -> x + 0.001 * randn -> Normalize           (`main/train_clip_imagenet.py:27-36`)
// and the per-batch device Normalize of `training/ad_trainer.py:413-425`, as ONE HBM-bound gather kernel over a uint8 NHWC
// image set that stays resident in HBM (CIFAR-10's 50 000 training images are 150 MB of the 288 GB): per step the host
// sends only (image index, crop origin, flip) per sample; the PIL work in DataLoader workers (`ad_trainer.py:103,385`)
// disappears.  Resize (bilinear / bicubic with Pillow's antialiasing) and ColorJitter are the kernels at the end of this file.
// The noise is counter-based: element e of batch slot b draws from splitmix64(seed * 2^40 + b * 2^18 + e) by Box-Muller,
// so a step is reproducible from (seed, crop parameters) and restatable on the CPU (oracle/augment.py).
#include "common.h"
#include <math.h>
#include <stdlib.h>

namespace {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the source pixel (3 bytes) of output pixel (y, x) of batch slot b, NULL in the zero padding
__device__ __forceinline__ const uint8_t* crop_flip_src(const uint8_t* __restrict__ src, const int32_t* __restrict__ params, int b, int y,
                                                        int x, int Hs, int Ws, int Wo, int flip_first) {
    const int idx = params[b * 4 + 0], top = params[b * 4 + 1], left = params[b * 4 + 2], flip = params[b * 4 + 3];
    const int sy = top + y;
    int sx;
    if (flip_first) sx = flip ? Ws - 1 - (left + x) : left + x;          // flip the source, then crop
    else sx = left + (flip ? Wo - 1 - x : x);                            // crop, then flip the crop
    if (sy < 0 || sy >= Hs || sx < 0 || sx >= Ws) return nullptr;
    return src + (((size_t)idx * Hs + sy) * Ws + sx) * 3;
}

// one thread per output pixel (img, y, x): 3 source bytes -> 3 floats in the 3 NCHW planes (coalesced along x)
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ params,
                                                      const float* __restrict__ mean, const float* __restrict__ stdv,
                                                      float* __restrict__ out, int n, int Hs, int Ws, int Ho, int Wo,
                                                      int flip_first, float noise_std, unsigned long long seed) {
    const size_t total = (size_t)n * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), b = (int)(i / ((size_t)Wo * Ho));
        const uint8_t* p = crop_flip_src(src, params, b, y, x, Hs, Ws, Wo, flip_first);
        float v[3] = {0.f, 0.f, 0.f};                                        // RandomCrop pads with 0
        if (p) {
            v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float a = v[c] / 255.0f;                                         // ToTensor
            if (noise_std > 0.f) {
                const unsigned long long e = ((unsigned long long)c * Ho + y) * Wo + x;
                const unsigned long long z = splitmix64((seed << 40) + ((unsigned long long)b << 18) + e);
                const float u1 = (float)((z >> 40) + 1ull) * (1.0f / 16777216.0f);          // (0, 1]
                const float u2 = (float)((z >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);   // [0, 1)
                a += noise_std * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
            }
            if (mean) a = (a - mean[c]) / stdv[c];
            out[(((size_t)b * 3 + c) * Ho + y) * Wo + x] = a;
        }
    }
}

}  // namespace

// ---- one-channel form (the 28 x 28 tasks, main/train_fmnist.py:31-38, main/train_mnist.py): with one byte per pixel a thread per
// pixel wastes the gather, so a thread takes 4 adjacent output pixels of a row.  Along a row the source column is s0 + dir * x
// (dir = -1 when flipped), so where the 4 columns lie inside the image they are 4 consecutive bytes: one load.
namespace {

// v[k] = the source byte of output pixel (y, x0 + k) of batch slot b, k = 0..3; 0 in the zero padding, for x0 + k >= Wo (never
// stored) and for a slot whose image index lies outside the set
__device__ __forceinline__ void gather4_c1(const uint8_t* __restrict__ src, long long n_src, const int32_t* __restrict__ params, int b,
                                           int y, int x0, int Hs, int Ws, int Wo, int flip_first, int v[4]) {
    const int idx = params[b * 4 + 0], top = params[b * 4 + 1], left = params[b * 4 + 2], flip = params[b * 4 + 3];
    v[0] = v[1] = v[2] = v[3] = 0;
    const int sy = top + y;
    if (sy < 0 || sy >= Hs || idx < 0 || (long long)idx >= n_src) return;
    int s0, dir;                                                         // source column of output column x: s0 + dir * x
    if (!flip) { s0 = left; dir = 1; }
    else if (flip_first) { s0 = Ws - 1 - left; dir = -1; }               // flip the source, then crop
    else { s0 = left + Wo - 1; dir = -1; }                               // crop, then flip the crop
    const uint8_t* row = src + ((size_t)idx * Hs + sy) * Ws;
    const int sa = s0 + dir * x0, sb = s0 + dir * (x0 + 3);              // first and last of the 4 source columns
    const int lo = dir > 0 ? sa : sb;
    if (x0 + 3 < Wo && lo >= 0 && lo + 3 < Ws) {
        unsigned w;
        __builtin_memcpy(&w, row + lo, 4);                               // any alignment: left is arbitrary
        if (dir < 0) w = __builtin_bswap32(w);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                        // a padded border, or the ragged end of a row
        const int sx = sa + dir * k;
        if (x0 + k < Wo && sx >= 0 && sx < Ws) v[k] = row[sx];
    }
}

// thread per (slot, row, quad of 4 columns); VEC: Wo % 4 == 0 and `out` 16-byte aligned, the quad leaves as one float4
template <bool VEC>
__global__ __launch_bounds__(256) void augment_c1_kernel(const uint8_t* __restrict__ src, long long n_src, const int32_t* __restrict__ params,
                                                         const float* __restrict__ mean, const float* __restrict__ stdv,
                                                         float* __restrict__ out, int n, int Hs, int Ws, int Ho, int Wo,
                                                         int flip_first, float noise_std, unsigned long long seed) {
    const int Q = (Wo + 3) / 4;
    const size_t total = (size_t)n * Ho * Q;
    const float m = mean ? mean[0] : 0.f, s = mean ? stdv[0] : 1.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % Q) * 4, y = (int)((i / Q) % Ho), b = (int)(i / ((size_t)Q * Ho));
        int v[4];
        gather4_c1(src, n_src, params, b, y, x0, Hs, Ws, Wo, flip_first, v);
        float a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[k] = (float)v[k] / 255.0f;                                     // ToTensor
            if (noise_std > 0.f) {                                           // the rule of augment_kernel with c = 0
                const unsigned long long e = (unsigned long long)y * Wo + (x0 + k);
                const unsigned long long z = splitmix64((seed << 40) + ((unsigned long long)b << 18) + e);
                const float u1 = (float)((z >> 40) + 1ull) * (1.0f / 16777216.0f);          // (0, 1]
                const float u2 = (float)((z >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);   // [0, 1)
                a[k] += noise_std * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
            }
            if (mean) a[k] = (a[k] - m) / s;
        }
        float* o = out + ((size_t)b * Ho + y) * Wo + x0;
        if (VEC) *reinterpret_cast<float4*>(o) = make_float4(a[0], a[1], a[2], a[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < Wo) o[k] = a[k];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void crop_flip_c1_kernel(const uint8_t* __restrict__ src, long long n_src, const int32_t* __restrict__ params,
                                                           uint8_t* __restrict__ out, int n, int Hs, int Ws, int Ho, int Wo, int flip_first) {
    const int Q = (Wo + 3) / 4;
    const size_t total = (size_t)n * Ho * Q;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % Q) * 4, y = (int)((i / Q) % Ho), b = (int)(i / ((size_t)Q * Ho));
        int v[4];
        gather4_c1(src, n_src, params, b, y, x0, Hs, Ws, Wo, flip_first, v);
        uint8_t* o = out + ((size_t)b * Ho + y) * Wo + x0;
        if (VEC) *reinterpret_cast<unsigned*>(o) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < Wo) o[k] = (uint8_t)v[k];
        }
    }
}

}  // namespace

extern "C" int eoe_augment_batch_c(const uint8_t* src, int64_t n_src, int Hs, int Ws, int C, const int32_t* params, const float* mean,
                                   const float* stdv, float* out, int n, int Ho, int Wo, int flip_first, float noise_std,
                                   uint64_t seed, void* stream) {
    EOE_CHECK_ARG(C == 1 || C == 3, "augment_batch: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(src && params && out && n_src > 0 && n > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "augment_batch: bad args");
    EOE_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "augment_batch: mean/std must both be given or both NULL");
    EOE_CHECK_ARG(n < (1 << 22) && (size_t)3 * Ho * Wo < (1u << 18) && seed < (1ull << 24) && noise_std >= 0.f,
                  "augment_batch: n < 2^22, 3*Ho*Wo < 2^18, seed < 2^24 (the counter layout of the noise generator)");
    ProfScope ps("augment_batch", 0, (double)C * n * Ho * Wo + 4.0 * C * n * Ho * Wo, stream);
    if (C == 3) {
        size_t g = ((size_t)n * Ho * Wo + 255) / 256;
        if (g > 8192) g = 8192;
        hipLaunchKernelGGL(augment_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, params, mean, stdv, out, n, Hs, Ws,
                           Ho, Wo, flip_first, noise_std, (unsigned long long)seed);
    } else {
        size_t g = ((size_t)n * Ho * ((Wo + 3) / 4) + 255) / 256;
        if (g > 8192) g = 8192;
        const bool vec = Wo % 4 == 0 && (uintptr_t)out % 16 == 0;
        hipLaunchKernelGGL(vec ? augment_c1_kernel<true> : augment_c1_kernel<false>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                           src, (long long)n_src, params, mean, stdv, out, n, Hs, Ws, Ho, Wo, flip_first, noise_std, (unsigned long long)seed);
    }
    EOE_CHECK_LAUNCH("augment_batch");
    return 0;
}

extern "C" int eoe_augment_batch(const uint8_t* src, int64_t n_src, int Hs, int Ws, const int32_t* params, const float* mean,
                                 const float* stdv, float* out, int n, int Ho, int Wo, int flip_first, float noise_std,
                                 uint64_t seed, void* stream) {
    return eoe_augment_batch_c(src, n_src, Hs, Ws, 3, params, mean, stdv, out, n, Ho, Wo, flip_first, noise_std, seed, stream);
}

// the crop / flip of eoe_augment_batch alone, uint8 NHWC out: the PIL-stage image that a uint8 filter (the sharpen MSM) sees
// between the reference's RandomCrop / RandomHorizontalFlip and ToTensor
namespace {
__global__ __launch_bounds__(256) void crop_flip_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ params,
                                                        uint8_t* __restrict__ out, int n, int Hs, int Ws, int Ho, int Wo, int flip_first) {
    const size_t total = (size_t)n * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), b = (int)(i / ((size_t)Wo * Ho));
        const uint8_t* p = crop_flip_src(src, params, b, y, x, Hs, Ws, Wo, flip_first);
        uint8_t* o = out + i * 3;
        o[0] = p ? p[0] : 0; o[1] = p ? p[1] : 0; o[2] = p ? p[2] : 0;
    }
}
}  // namespace

extern "C" int eoe_crop_flip_u8_c(const uint8_t* src, int64_t n_src, int Hs, int Ws, int C, const int32_t* params, uint8_t* out, int n,
                                  int Ho, int Wo, int flip_first, void* stream) {
    EOE_CHECK_ARG(C == 1 || C == 3, "crop_flip_u8: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(src && params && out && n_src > 0 && n > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, "crop_flip_u8: bad args");
    EOE_CHECK_ARG((const void*)src != (const void*)out, "crop_flip_u8: out must not alias src");
    ProfScope ps("crop_flip_u8", 0, 2.0 * C * n * Ho * Wo, stream);
    if (C == 3) {
        size_t g = ((size_t)n * Ho * Wo + 255) / 256;
        if (g > 8192) g = 8192;
        hipLaunchKernelGGL(crop_flip_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, params, out, n, Hs, Ws, Ho, Wo,
                           flip_first);
    } else {
        size_t g = ((size_t)n * Ho * ((Wo + 3) / 4) + 255) / 256;
        if (g > 8192) g = 8192;
        const bool vec = Wo % 4 == 0 && (uintptr_t)out % 4 == 0;
        hipLaunchKernelGGL(vec ? crop_flip_c1_kernel<true> : crop_flip_c1_kernel<false>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                           src, (long long)n_src, params, out, n, Hs, Ws, Ho, Wo, flip_first);
    }
    EOE_CHECK_LAUNCH("crop_flip_u8");
    return 0;
}

extern "C" int eoe_crop_flip_u8(const uint8_t* src, int64_t n_src, int Hs, int Ws, const int32_t* params, uint8_t* out, int n, int Ho,
                                int Wo, int flip_first, void* stream) {
    return eoe_crop_flip_u8_c(src, n_src, Hs, Ws, 3, params, out, n, Ho, Wo, flip_first, stream);
}

// ---- ragged sets (main/train_imagenet.py:30-34, train_cub.py, train_dtd.py, train_mvtec.py, train_custom.py: Resize(256) keeps the
// aspect ratio, so every image has its own shape): the images lie back to back in one uint8 arena, image i at arena + offsets[i]
// (int64), row-major HWC with (H, W) = sizes[2 i], sizes[2 i + 1].  The kernels above compute a slot's image from index * H * W * C;
// these look (offset, H, W) up.  A workgroup works on ONE slot (blockIdx.x / bps), so params and both table entries are
// workgroup-uniform: the compiler reads them with scalar loads once, in front of the pixel loop, not per pixel.  bps workgroups
// share a slot's outputs with a stride loop, which keeps the launch as wide as the uniform kernels' (8192 workgroups) at 256
// slots.  No row is assumed aligned (W * C is odd for most images): the loads are byte loads, or the 4-byte memcpy of gather4_c1.
// Statements of the fp32 tail are those of augment_kernel / augment_c1_kernel, in front of the `fp contract(off)` pragma below
// like them: the results are equal bit for bit (tests/test_gpu_ragged.py).
namespace {

struct RaggedImage { const uint8_t* base; int H, W; };                  // base NULL: the index lies outside the set -> all padding

__device__ __forceinline__ RaggedImage ragged_image(const uint8_t* __restrict__ arena, const long long* __restrict__ offsets,
                                                    const int32_t* __restrict__ sizes, long long n_src, int idx) {
    RaggedImage im = {nullptr, 0, 0};
    if (idx >= 0 && (long long)idx < n_src) {
        im.base = arena + offsets[idx];
        im.H = sizes[2 * idx];
        im.W = sizes[2 * idx + 1];
    }
    return im;
}

// source column of output column x of a slot: s0 + dir * x (crop_flip_src's two flip orders)
__device__ __forceinline__ void ragged_columns(int left, int flip, int flip_first, int Ws, int Wo, int& s0, int& dir) {
    if (!flip) { s0 = left; dir = 1; }
    else if (flip_first) { s0 = Ws - 1 - left; dir = -1; }               // flip the source, then crop
    else { s0 = left + Wo - 1; dir = -1; }                               // crop, then flip the crop
}

// ToTensor, noise and Normalize of byte v, element e of slot b, channel c: augment_kernel's statements
__device__ __forceinline__ float ragged_to_float(int v, unsigned long long e, int b, int c, const float* __restrict__ mean,
                                                 const float* __restrict__ stdv, float noise_std, unsigned long long seed) {
    float a = (float)v / 255.0f;                                             // ToTensor
    if (noise_std > 0.f) {
        const unsigned long long z = splitmix64((seed << 40) + ((unsigned long long)b << 18) + e);
        const float u1 = (float)((z >> 40) + 1ull) * (1.0f / 16777216.0f);          // (0, 1]
        const float u2 = (float)((z >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);   // [0, 1)
        a += noise_std * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
    }
    if (mean) a = (a - mean[c]) / stdv[c];
    return a;
}

// gather4_c1 on a row that is already looked up (NULL: padding): v[k] = the byte under output column x0 + k
__device__ __forceinline__ void ragged_gather4(const uint8_t* __restrict__ row, int Ws, int s0, int dir, int x0, int Wo, int v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0;
    if (!row) return;
    const int sa = s0 + dir * x0, sb = s0 + dir * (x0 + 3);
    const int lo = dir > 0 ? sa : sb;
    if (x0 + 3 < Wo && lo >= 0 && lo + 3 < Ws) {
        unsigned w;
        __builtin_memcpy(&w, row + lo, 4);                               // any alignment
        if (dir < 0) w = __builtin_bswap32(w);
        v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sx = sa + dir * k;
        if (x0 + k < Wo && sx >= 0 && sx < Ws) v[k] = row[sx];
    }
}

// three channels, a thread per output pixel of its slot; F32: fp32 NCHW with the tail, else uint8 NHWC
template <bool F32>
__global__ __launch_bounds__(256) void ragged_c3_kernel(const uint8_t* __restrict__ arena, const long long* __restrict__ offsets,
                                                        const int32_t* __restrict__ sizes, long long n_src, const int32_t* __restrict__ params,
                                                        const float* __restrict__ mean, const float* __restrict__ stdv, void* __restrict__ out_,
                                                        int bps, int Ho, int Wo, int flip_first, float noise_std, unsigned long long seed) {
    const int b = blockIdx.x / bps, part = blockIdx.x % bps;
    const int idx = params[b * 4 + 0], top = params[b * 4 + 1], left = params[b * 4 + 2], flip = params[b * 4 + 3];
    const RaggedImage im = ragged_image(arena, offsets, sizes, n_src, idx);
    int s0, dir;
    ragged_columns(left, flip, flip_first, im.W, Wo, s0, dir);
    const int total = Ho * Wo;
    for (int i = part * 256 + (int)threadIdx.x; i < total; i += bps * 256) {
        const int x = i % Wo, y = i / Wo;
        const int sy = top + y, sx = s0 + dir * x;
        int v[3] = {0, 0, 0};                                                // RandomCrop pads with 0
        if (im.base && sy >= 0 && sy < im.H && sx >= 0 && sx < im.W) {
            const uint8_t* p = im.base + ((size_t)sy * im.W + sx) * 3;
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        }
        if (F32) {
            float* out = static_cast<float*>(out_);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned long long e = ((unsigned long long)c * Ho + y) * Wo + x;
                out[(((size_t)b * 3 + c) * Ho + y) * Wo + x] = ragged_to_float(v[c], e, b, c, mean, stdv, noise_std, seed);
            }
        } else {
            uint8_t* o = static_cast<uint8_t*>(out_) + ((size_t)b * total + i) * 3;
            o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
        }
    }
}

// one channel, a thread per quad of 4 output columns of its slot (augment_c1_kernel / crop_flip_c1_kernel); VEC: the quad leaves as
// one float4 (F32) or one 4-byte word
template <bool F32, bool VEC>
__global__ __launch_bounds__(256) void ragged_c1_kernel(const uint8_t* __restrict__ arena, const long long* __restrict__ offsets,
                                                        const int32_t* __restrict__ sizes, long long n_src, const int32_t* __restrict__ params,
                                                        const float* __restrict__ mean, const float* __restrict__ stdv, void* __restrict__ out_,
                                                        int bps, int Ho, int Wo, int flip_first, float noise_std, unsigned long long seed) {
    const int b = blockIdx.x / bps, part = blockIdx.x % bps;
    const int idx = params[b * 4 + 0], top = params[b * 4 + 1], left = params[b * 4 + 2], flip = params[b * 4 + 3];
    const RaggedImage im = ragged_image(arena, offsets, sizes, n_src, idx);
    int s0, dir;
    ragged_columns(left, flip, flip_first, im.W, Wo, s0, dir);
    const int Q = (Wo + 3) / 4, total = Ho * Q;
    for (int i = part * 256 + (int)threadIdx.x; i < total; i += bps * 256) {
        const int x0 = (i % Q) * 4, y = i / Q;
        const int sy = top + y;
        const uint8_t* row = (im.base && sy >= 0 && sy < im.H) ? im.base + (size_t)sy * im.W : nullptr;
        int v[4];
        ragged_gather4(row, im.W, s0, dir, x0, Wo, v);
        const size_t at = ((size_t)b * Ho + y) * Wo + x0;
        if (F32) {
            float a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = ragged_to_float(v[k], (unsigned long long)y * Wo + (x0 + k), b, 0, mean, stdv, noise_std, seed);
            float* o = static_cast<float*>(out_) + at;
            if (VEC) *reinterpret_cast<float4*>(o) = make_float4(a[0], a[1], a[2], a[3]);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x0 + k < Wo) o[k] = a[k];
            }
        } else {
            uint8_t* o = static_cast<uint8_t*>(out_) + at;
            if (VEC) *reinterpret_cast<unsigned*>(o) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x0 + k < Wo) o[k] = (uint8_t)v[k];
            }
        }
    }
}

// workgroups per slot: enough that every thread has an element, at most about 8192 workgroups in all (the uniform kernels' cap)
int ragged_bps(int n, size_t per_slot) {
    size_t bps = (per_slot + 255) / 256, cap = 8192 / (size_t)n;
    if (bps > cap) bps = cap;
    return bps < 1 ? 1 : (int)bps;
}

template <bool F32>
void ragged_crop_launch(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src, int C, const int32_t* params,
                        const float* mean, const float* stdv, void* out, int n, int Ho, int Wo, int flip_first, float noise_std,
                        uint64_t seed, void* stream) {
    const long long* off = reinterpret_cast<const long long*>(offsets);
    if (C == 3) {
        const int bps = ragged_bps(n, (size_t)Ho * Wo);
        hipLaunchKernelGGL(ragged_c3_kernel<F32>, dim3((unsigned)((size_t)n * bps)), dim3(256), 0, (hipStream_t)stream, arena, off, sizes,
                           (long long)n_src, params, mean, stdv, out, bps, Ho, Wo, flip_first, noise_std, (unsigned long long)seed);
    } else {
        const int bps = ragged_bps(n, (size_t)Ho * ((Wo + 3) / 4));
        const bool vec = Wo % 4 == 0 && (uintptr_t)out % (F32 ? 16 : 4) == 0;
        hipLaunchKernelGGL((vec ? ragged_c1_kernel<F32, true> : ragged_c1_kernel<F32, false>), dim3((unsigned)((size_t)n * bps)), dim3(256), 0,
                           (hipStream_t)stream, arena, off, sizes, (long long)n_src, params, mean, stdv, out, bps, Ho, Wo, flip_first,
                           noise_std, (unsigned long long)seed);
    }
}

}  // namespace

extern "C" int eoe_ragged_augment_batch(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src, int C,
                                        const int32_t* params, const float* mean, const float* stdv, float* out, int n, int Ho, int Wo,
                                        int flip_first, float noise_std, uint64_t seed, void* stream) {
    EOE_CHECK_ARG(C == 1 || C == 3, "ragged_augment_batch: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(n >= 0 && n_src > 0 && Ho > 0 && Wo > 0, "ragged_augment_batch: bad args");
    if (n == 0) return 0;
    EOE_CHECK_ARG(arena && offsets && sizes && params && out, "ragged_augment_batch: bad args");
    EOE_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "ragged_augment_batch: mean/std must both be given or both NULL");
    EOE_CHECK_ARG(n < (1 << 22) && (size_t)3 * Ho * Wo < (1u << 18) && seed < (1ull << 24) && noise_std >= 0.f,
                  "ragged_augment_batch: n < 2^22, 3*Ho*Wo < 2^18, seed < 2^24 (the counter layout of the noise generator)");
    ProfScope ps("ragged_augment", 0, (double)C * n * Ho * Wo + 4.0 * C * n * Ho * Wo, stream);
    ragged_crop_launch<true>(arena, offsets, sizes, n_src, C, params, mean, stdv, out, n, Ho, Wo, flip_first, noise_std, seed, stream);
    EOE_CHECK_LAUNCH("ragged_augment_batch");
    return 0;
}

extern "C" int eoe_ragged_crop_flip_u8(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src, int C,
                                       const int32_t* params, uint8_t* out, int n, int Ho, int Wo, int flip_first, void* stream) {
    EOE_CHECK_ARG(C == 1 || C == 3, "ragged_crop_flip_u8: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(n >= 0 && n_src > 0 && Ho > 0 && Wo > 0, "ragged_crop_flip_u8: bad args");
    if (n == 0) return 0;
    EOE_CHECK_ARG(arena && offsets && sizes && params && out, "ragged_crop_flip_u8: bad args");
    EOE_CHECK_ARG((const void*)arena != (const void*)out, "ragged_crop_flip_u8: out must not alias the arena");
    EOE_CHECK_ARG(n < (1 << 22) && (size_t)Ho * Wo < (1u << 28), "ragged_crop_flip_u8: n < 2^22 and Ho*Wo < 2^28");
    ProfScope ps("ragged_crop_flip", 0, 2.0 * C * n * Ho * Wo, stream);
    ragged_crop_launch<false>(arena, offsets, sizes, n_src, C, params, nullptr, nullptr, out, n, Ho, Wo, flip_first, 0.f, 0, stream);
    EOE_CHECK_LAUNCH("ragged_crop_flip_u8");
    return 0;
}

// ---- CLIP's per-sample upsample inside the chain (main/train_clip_cifar.py:26-35, train_clip_fmnist.py:27-36, train_clip_mnist.py:25-29):
//   ... RandomCrop(S, padding) -> RandomHorizontalFlip -> Resize(P, BICUBIC) -> CenterCrop(P) -> convert("RGB") -> ToTensor -> noise -> Normalize
// The resize comes after the random crop / flip, so it runs per sample per step.  A slot's source is only S x S x C bytes (3 KB at
// 32 x 32 x 3), so the whole chain of a slot runs out of LDS and the only HBM traffic that matters is the fp32 store.  A workgroup
// takes one BAND of R output rows of one slot (n * bands workgroups: 256 slots alone would leave most of the chip idle):
//   1  gathers the few crop rows its band needs (rows [r0, r0 + nr), read off the vertical tap table) into LDS, by the crop / flip
//      rules of eoe_crop_flip_u8_c, zero padding; loads are unconditional on clamped addresses, the padding is a select
//   2  Pillow's horizontal pass on those rows, rounded to uint8 as Pillow rounds it, into LDS planes [C][nr][P]
//   3  the vertical pass for 4 adjacent outputs of one row and plane per thread (one 4-byte LDS read per tap), the L -> RGB
//      replication, then ToTensor / noise / Normalize in the statements of augment_kernel, one 16-byte store
// Stages 1-3 up to the byte are integer arithmetic, the arithmetic of resize_pass_kernel below.  This kernel stands in front of
// the `fp contract(off)` pragma further down on purpose: augment_kernel is compiled with contraction, and the fp32 of this kernel is
// that of the composed chain bit for bit only under the same setting.
namespace {

constexpr int AR_PRECISION_BITS = 32 - 8 - 2;                            // Resample.c PRECISION_BITS (RESIZE_PRECISION_BITS below)

__device__ __forceinline__ int ar_clip8(int ss) {
    ss >>= AR_PRECISION_BITS;
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

// ToTensor, noise and Normalize of byte v at (c, y, x) of slot b of an [., 3, P, P] batch: augment_kernel's statements
__device__ __forceinline__ float ar_to_float(int v, int c, int y, int x, int P, int b, const float* __restrict__ mean,
                                             const float* __restrict__ stdv, float noise_std, unsigned long long seed) {
    float a = (float)v / 255.0f;                                             // ToTensor
    if (noise_std > 0.f) {
        const unsigned long long e = ((unsigned long long)c * P + y) * P + x;
        const unsigned long long z = splitmix64((seed << 40) + ((unsigned long long)b << 18) + e);
        const float u1 = (float)((z >> 40) + 1ull) * (1.0f / 16777216.0f);          // (0, 1]
        const float u2 = (float)((z >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);   // [0, 1)
        a += noise_std * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
    }
    if (mean) a = (a - mean[c]) / stdv[c];
    return a;
}

// C source channels, KS taps per output (3 bilinear, 5 bicubic: an upsample's support is the filter's own).  Dynamic LDS:
// crop [nr_cap][S * C] (crop_bytes, a multiple of 16), then hbuf [C][nr_cap][Pp], Pp = P rounded up to 4.  Every index taken from
// the tap tables is clamped to the buffers, so a wrong table gives wrong pixels, never an access outside them.
template <int C, int KS>
__global__ __launch_bounds__(256) void augment_resize_kernel(const uint8_t* __restrict__ src, long long n_src, const int32_t* __restrict__ params,
                                                             const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                             const float* __restrict__ mean, const float* __restrict__ stdv,
                                                             float* __restrict__ out, int Hs, int Ws, int S, int P, int bands, int R,
                                                             int nr_cap, int crop_bytes, int flip_first, int vec, float noise_std,
                                                             unsigned long long seed) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ar_lds[];
    uint8_t* crop = ar_lds;
    uint8_t* hbuf = ar_lds + crop_bytes;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / bands, band = blockIdx.x % bands;
    const int y0 = band * R, y1 = min(y0 + R, P);                        // this band's output rows [y0, y1)
    const int Pp = (P + 3) & ~3;
    // the source rows the band's vertical taps reach: first row of its first output, past-the-last row of its last (both grow with y)
    const int r0 = min(max(bounds[2 * y0], 0), S - 1);
    const int rend = min(bounds[2 * (y1 - 1)] + bounds[2 * (y1 - 1) + 1], S);
    const int nr = min(max(rend - r0, 1), nr_cap);

    // 1: gather
    const int idx = params[b * 4 + 0], top = params[b * 4 + 1], left = params[b * 4 + 2], flip = params[b * 4 + 3];
    const bool in_set = idx >= 0 && (long long)idx < n_src;
    const uint8_t* img = src + (size_t)(in_set ? idx : 0) * Hs * Ws * C;
    for (int i = tid; i < nr * S; i += 256) {
        const int r = i / S, x = i - r * S;
        const long long sy = (long long)top + r0 + r;
        long long sx;
        if (flip_first) sx = flip ? (long long)Ws - 1 - ((long long)left + x) : (long long)left + x;    // flip the source, then crop
        else sx = (long long)left + (flip ? S - 1 - x : x);                                             // crop, then flip the crop
        const bool ok = in_set && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
        const int cy = (int)min(max(sy, 0ll), (long long)Hs - 1), cx = (int)min(max(sx, 0ll), (long long)Ws - 1);
        const uint8_t* p = img + ((size_t)cy * Ws + cx) * C;
        int v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p[c];
#pragma unroll
        for (int c = 0; c < C; ++c) crop[i * C + c] = (uint8_t)(ok ? v[c] : 0);                         // RandomCrop pads with 0
    }
    __syncthreads();

    // 2: horizontal pass, a thread per output column: its taps stay in registers over the rows and channels
    for (int x = tid; x < P; x += 256) {
        const int xmin = min(max(bounds[2 * x], 0), S - 1);
        const int cnt = min(max(bounds[2 * x + 1], 0), min(KS, S - xmin));
        int k[KS], off[KS];
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            const int t = kk[x * KS + j];
            k[j] = j < cnt ? t : 0;
            off[j] = min(xmin + j, S - 1) * C;
        }
        for (int r = 0; r < nr; ++r) {
            const uint8_t* row = crop + r * S * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                int ss = 1 << (AR_PRECISION_BITS - 1);
#pragma unroll
                for (int j = 0; j < KS; ++j) ss += (int)row[off[j] + c] * k[j];
                hbuf[(c * nr_cap + r) * Pp + x] = (uint8_t)ar_clip8(ss);
            }
        }
    }
    __syncthreads();

    // 3: vertical pass and the fp32 tail; quads run along x first, so a wave stores 1 KiB of consecutive floats
    const int Q = Pp / 4, rows = y1 - y0;
    const int nq = 3 * rows * Q;
    for (int q = tid; q < nq; q += 256) {
        const int xq = q % Q, yy = (q / Q) % rows, co = q / (Q * rows);
        const int cs = C == 3 ? co : 0;                                  // convert("RGB") of an L image: the byte, three times
        const int y = y0 + yy, x0 = xq * 4;
        const int ymin = min(max(bounds[2 * y], 0), S - 1);
        const int cnt = min(max(bounds[2 * y + 1], 0), min(KS, S - ymin));
        int ss[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ss[k] = 1 << (AR_PRECISION_BITS - 1);
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            const int t = kk[y * KS + j];
            const int kj = j < cnt ? t : 0;
            const int rr = min(max(ymin + j - r0, 0), nr - 1);
            const unsigned w = *reinterpret_cast<const unsigned*>(hbuf + (cs * nr_cap + rr) * Pp + x0);
            ss[0] += (int)(w & 255u) * kj; ss[1] += (int)((w >> 8) & 255u) * kj;
            ss[2] += (int)((w >> 16) & 255u) * kj; ss[3] += (int)(w >> 24) * kj;
        }
        float a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = ar_to_float(ar_clip8(ss[k]), co, y, x0 + k, P, b, mean, stdv, noise_std, seed);
        float* o = out + (((size_t)b * 3 + co) * P + y) * P + x0;
        if (vec) *reinterpret_cast<float4*>(o) = make_float4(a[0], a[1], a[2], a[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < P) o[k] = a[k];
        }
    }
}

}  // namespace

extern "C" int eoe_augment_resize_batch(const uint8_t* src, int64_t n_src, int Hs, int Ws, int C, const int32_t* params, int crop_h,
                                        int crop_w, int n_px, int filter, const int32_t* bounds, const int32_t* kk, const float* mean,
                                        const float* stdv, float* out, int n, int flip_first, float noise_std, uint64_t seed,
                                        void* stream) {
    EOE_CHECK_ARG(C == 1 || C == 3, "augment_resize_batch: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(src && params && bounds && kk && out && n_src > 0 && n > 0 && Hs > 0 && Ws > 0 && crop_h > 0 && crop_w > 0 && n_px > 0,
                  "augment_resize_batch: bad args");
    EOE_CHECK_ARG(filter == EOE_RESIZE_BILINEAR || filter == EOE_RESIZE_BICUBIC,
                  "augment_resize_batch: filter must be EOE_RESIZE_BILINEAR or EOE_RESIZE_BICUBIC, not %d", filter);
    EOE_CHECK_ARG(crop_h == crop_w, "augment_resize_batch: the crop must be square, not %d x %d (CenterCrop after Resize is the identity "
                  "only then)", crop_h, crop_w);
    EOE_CHECK_ARG(crop_h <= 64 && n_px <= 256, "augment_resize_batch: crop <= 64 and n_px <= 256 (a band's rows live in LDS), not %d -> %d",
                  crop_h, n_px);
    EOE_CHECK_ARG(n_px >= crop_h, "augment_resize_batch: %d -> %d is a downscale; only upsampling (n_px >= crop) is built", crop_h, n_px);
    EOE_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "augment_resize_batch: mean/std must both be given or both NULL");
    EOE_CHECK_ARG(n < (1 << 22) && (size_t)3 * n_px * n_px < (1u << 18) && seed < (1ull << 24) && noise_std >= 0.f,
                  "augment_resize_batch: n < 2^22, 3*n_px*n_px < 2^18, seed < 2^24 (the counter layout of the noise generator)");
    const int S = crop_h, P = n_px;
    const int support = filter == EOE_RESIZE_BILINEAR ? 1 : 2;          // not stretched: the scale is <= 1
    // bands: about 2048 workgroups in flight where the batch allows it, and at least 8 output rows per band
    int bands = (2048 + n - 1) / n;
    if (bands > P / 8) bands = P / 8;
    if (bands < 1) bands = 1;
    const int R = (P + bands - 1) / bands;
    bands = (P + R - 1) / R;
    // R consecutive outputs have their centres within (R - 1) * S / P source rows; each end reaches `support` rows further
    int nr_cap = (int)((long long)(R - 1) * S / P) + 2 * support + 2;
    if (nr_cap > S) nr_cap = S;
    const int Pp = (P + 3) & ~3;
    const int crop_bytes = (nr_cap * S * C + 15) & ~15;
    const size_t lds = (size_t)crop_bytes + (size_t)C * nr_cap * Pp;      // <= 12 KiB + 48 KiB at S = 64, P = 256, C = 3, one band
    EOE_CHECK_ARG(lds <= 64 * 1024, "augment_resize_batch: %zu bytes of LDS", lds);
    const int vec = P % 4 == 0 && (uintptr_t)out % 16 == 0;
    ProfScope ps("augment_resize_batch", 0, (double)C * n * S * S + 4.0 * 3 * n * P * P, stream);
    const dim3 grid((unsigned)((size_t)n * bands)), block(256);
#define EOE_AR_LAUNCH(CC, KS)                                                                                                      \
    hipLaunchKernelGGL((augment_resize_kernel<CC, KS>), grid, block, lds, (hipStream_t)stream, src, (long long)n_src, params, bounds, kk, \
                       mean, stdv, out, Hs, Ws, S, P, bands, R, nr_cap, crop_bytes, flip_first, vec, noise_std, (unsigned long long)seed)
    if (C == 3) {
        if (support == 2) EOE_AR_LAUNCH(3, 5); else EOE_AR_LAUNCH(3, 3);
    } else {
        if (support == 2) EOE_AR_LAUNCH(1, 5); else EOE_AR_LAUNCH(1, 3);
    }
#undef EOE_AR_LAUNCH
    EOE_CHECK_LAUNCH("augment_resize_batch");
    return 0;
}

// Grayscale(1) (main/train_fmnist.py:32; torchvision hands it to Pillow's Image.convert("L"), libImaging/Convert.c rgb2l): uint8 NHWC
// [., 3] -> [., 1], L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, byte for byte.  Deterministic and first in the chain, so a resident
// set is converted once.  A thread takes 16 pixels: three 16-byte loads, one 16-byte store; the pixels past the last whole 16 (all of
// them when a pointer is not 16-byte aligned) go one per thread.
namespace {
__device__ __forceinline__ unsigned rgb_byte(const unsigned* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

__global__ __launch_bounds__(256) void grayscale_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n_vec, size_t n_px) {
    const size_t total = n_vec + (n_px - n_vec * 16);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        if (i < n_vec) {
            const uint4* p = reinterpret_cast<const uint4*>(src) + i * 3;
            const uint4 q0 = p[0], q1 = p[1], q2 = p[2];
            const unsigned w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
            unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned l = (rgb_byte(w, 3 * k) * 19595u + rgb_byte(w, 3 * k + 1) * 38470u + rgb_byte(w, 3 * k + 2) * 7471u + 0x8000u) >> 16;
                o[k >> 2] |= l << ((k & 3) * 8);
            }
            reinterpret_cast<uint4*>(dst)[i] = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            const size_t px = n_vec * 16 + (i - n_vec);
            const uint8_t* p = src + px * 3;
            dst[px] = (uint8_t)(((unsigned)p[0] * 19595u + (unsigned)p[1] * 38470u + (unsigned)p[2] * 7471u + 0x8000u) >> 16);
        }
    }
}
}  // namespace

extern "C" int eoe_grayscale_u8(const uint8_t* src, uint8_t* dst, int64_t n_pixels, void* stream) {
    EOE_CHECK_ARG(src && dst && n_pixels > 0, "grayscale_u8: bad args");
    EOE_CHECK_ARG((const void*)src != (const void*)dst, "grayscale_u8: dst must not alias src");
    ProfScope ps("grayscale_u8", 0, 4.0 * (double)n_pixels, stream);
    const bool aligned = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const size_t n_vec = aligned ? (size_t)n_pixels / 16 : 0;
    const size_t total = n_vec + ((size_t)n_pixels - n_vec * 16);
    size_t g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(grayscale_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, dst, n_vec, (size_t)n_pixels);
    EOE_CHECK_LAUNCH("grayscale_u8");
    return 0;
}


// ------------------------------------------------------------------------------------------------------------------------
// Resize and ColorJitter (main/train_imagenet.py:30-31, main/train_clip_imagenet.py:28-29, main/train_cifar.py:32; CLIP's own
// preprocessing, clip_official/clip/clip.py:58-65).  In the reference these run on PIL images inside DataLoader workers:
// torchvision hands them to Pillow, so the arithmetic restated here is Pillow's 8-bit integer one and the results are equal to
// Pillow's byte for byte (tests/golden g14):
//   Image.resize            separable, horizontal then vertical on uint8, filter support stretched by the down-scaling factor
//                           (antialias), weights normalised in double and rounded to 22-bit fixed point (libImaging/Resample.c)
//   ImageEnhance.*          Image.blend(degenerate, image, factor): black / rounded mean gray / gray image (libImaging/Blend.c)
//   hue                     8-bit RGB -> HSV -> h + uint8(255 * factor) -> RGB (libImaging/Convert.c)
// ------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int RESIZE_PRECISION_BITS = 32 - 8 - 2;

double filter_bilinear(double x) { if (x < 0.0) x = -x; return x < 1.0 ? 1.0 - x : 0.0; }
double filter_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// one pass along `axis_len`: src [outer, axis_in, inner] -> dst [outer, axis_out, inner], uint8; thread per output byte
__global__ __launch_bounds__(256) void resize_pass_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const int32_t* __restrict__ bounds, const int32_t* __restrict__ kk,
                                                          int ksize, size_t outer, int axis_in, int axis_out, int inner) {
    const size_t total = outer * axis_out * inner;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int in = (int)(i % inner);
        const int xx = (int)((i / inner) % axis_out);
        const size_t o = i / ((size_t)inner * axis_out);
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const uint8_t* p = src + (o * axis_in + xmin) * inner + in;
        const int32_t* k = kk + (size_t)xx * ksize;
        int ss = 1 << (RESIZE_PRECISION_BITS - 1);
        for (int x = 0; x < cnt; ++x) ss += (int)p[(size_t)x * inner] * k[x];
        ss >>= RESIZE_PRECISION_BITS;
        dst[i] = (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
    }
}

// resize_pass_kernel over a ragged set, all images in ONE launch: image i is src + offs[2 i] viewed as [outer, axis_in, inner] ->
// dst + offs[2 i + 1] as [outer, axis_out, inner], with desc[8 i ..] = (outer, axis_in, axis_out, inner, bounds_at, kk_at, ksize, first);
// bounds_at / kk_at are positions in `taps`, the int32 arena that holds the host's eoe_resize_coeffs tables, one per distinct
// (in, out, filter) of the set.  bpi workgroups share an image's output bytes.  Integer arithmetic only; nothing about the taps is
// computed here.
// `first` is a window on the output axis (CLIP's CenterCrop after its Resize): the pass writes outputs [first, first + axis_out) of the
// full axis, packed as [outer, axis_out, inner]; bounds_at / kk_at still name the tables of the FULL axis, row `first + x` of them is
// output x.  With first = 0 and axis_out the full axis this is the whole pass.  ksize == 0 marks the pass Pillow skips (the full
// output axis equals axis_in; axis_in == axis_out alone cannot say so under a window): the window of the image is copied -- all of
// it without a window.  The source offset is signed and is added to the element's position before the pointer is formed: a
// vertical pass behind a horizontal one that wrote only the rows its taps touch is given the position source row 0 WOULD have,
// which may lie in front of the intermediate (ragged_resize_plan); no tap of the window reads there.
__global__ __launch_bounds__(256) void resize_pass_ragged_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                 const long long* __restrict__ offs, const int32_t* __restrict__ desc,
                                                                 const int32_t* __restrict__ taps, int bpi) {
    const int img = blockIdx.x / bpi, part = blockIdx.x % bpi;
    const int32_t* d = desc + (size_t)img * 8;
    const int outer = d[0], axis_in = d[1], axis_out = d[2], inner = d[3], ksize = d[6], win = d[7];
    const long long so = offs[2 * (size_t)img];
    uint8_t* o = dst + offs[2 * (size_t)img + 1];
    const size_t total = (size_t)outer * axis_out * inner;
    const size_t first = (size_t)part * 256 + threadIdx.x, step = (size_t)bpi * 256;
    if (ksize == 0) {
        if (win == 0 && axis_in == axis_out) {               // the whole image, as one run of bytes
            const uint8_t* s = src + so;
            for (size_t i = first; i < total; i += step) o[i] = s[i];
            return;
        }
        for (size_t i = first; i < total; i += step) {
            const int in = (int)(i % inner);
            const int xx = (int)((i / inner) % axis_out) + win;
            const size_t r = i / ((size_t)inner * axis_out);
            o[i] = src[so + (long long)((r * axis_in + xx) * inner + in)];
        }
        return;
    }
    const int32_t* bounds = taps + d[4];
    const int32_t* kk = taps + d[5];
    for (size_t i = first; i < total; i += step) {
        const int in = (int)(i % inner);
        const int xx = (int)((i / inner) % axis_out) + win;
        const size_t r = i / ((size_t)inner * axis_out);
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const uint8_t* p = src + (so + (long long)((r * axis_in + xmin) * inner + in));
        const int32_t* k = kk + (size_t)xx * ksize;
        int ss = 1 << (RESIZE_PRECISION_BITS - 1);
        for (int x = 0; x < cnt; ++x) ss += (int)p[(size_t)x * inner] * k[x];
        ss >>= RESIZE_PRECISION_BITS;
        o[i] = (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
    }
}

// Pillow's C code is compiled without fused multiply-adds; hipcc contracts a * b + c by default -- also through __fmul_rn /
// __fadd_rn, which are plain operators in HIP's headers -- and a blend that lands within one ulp of an integer then truncates
// to the neighbouring byte (saturation 0.99 on a gray level of 100: 100 - 99.00000095 = 0.99999905 -> 0 instead of 1)
#pragma clang fp contract(off)
// single IEEE operations compiled under the pragma above (HIP's __fmul_rn / __fadd_rn are header inlines that carry the default
// `contract` flag and still fuse)
__device__ __forceinline__ float add_(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_(float a, float b) { return a * b; }
__device__ __forceinline__ float div_(float a, float b) { return a / b; }

__device__ __forceinline__ int gray_l(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Blend.c: in1 + alpha * (in2 - in1) as separate float multiply and add (no fused multiply-add), truncated
__device__ __forceinline__ int blend_u8(int deg, int v, float alpha) {
    const float t = add_((float)deg, mul_(alpha, (float)(v - deg)));
    if (alpha >= 0.f && alpha <= 1.f) return (int)t & 255;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ void rgb2hsv_u8(int r, int g, int b, int& uh, int& us, int& uv) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    uv = maxc;
    if (minc == maxc) { uh = 0; us = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = div_(cr, (float)maxc);
    const float rc = div_((float)(maxc - r), cr), gc = div_((float)(maxc - g), cr), bc = div_((float)(maxc - b), cr);
    float h;
    if (r == maxc) h = sub_(bc, gc);
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    int ih = (int)((double)h * 255.0), is = (int)((double)s * 255.0);
    uh = ih < 0 ? 0 : (ih > 255 ? 255 : ih);
    us = is < 0 ? 0 : (is > 255 ? 255 : is);
}

__device__ __forceinline__ void hsv2rgb_u8(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) { r = g = b = v; return; }
    const float hf = div_(mul_((float)h, 6.0f), 255.0f);
    const int i = (int)floorf(hf);
    const float f = sub_(hf, (float)i);
    const float fs = div_((float)s, 255.0f);
    const float vf = (float)v;
    const int p = (int)floor((double)mul_(vf, sub_(1.0f, fs)) + 0.5);
    const int q = (int)floor((double)mul_(vf, sub_(1.0f, mul_(fs, f))) + 0.5);
    const int t = (int)floor((double)mul_(vf, sub_(1.0f, mul_(fs, sub_(1.0f, f)))) + 0.5);
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
    r = min(max(r, 0), 255); g = min(max(g, 0), 255); b = min(max(b, 0), 255);
}

// the ops of one image, in its order, applied to one pixel; `upto` = stop in front of the op with this code (4 = apply all)
__device__ __forceinline__ void jitter_pixel(int& r, int& g, int& b, const float* f, const int* order, int gray_mean, int upto) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int op = order[j];
        if (op == upto) return;
        if (op == 0) { r = blend_u8(0, r, f[0]); g = blend_u8(0, g, f[0]); b = blend_u8(0, b, f[0]); }
        else if (op == 1) { r = blend_u8(gray_mean, r, f[1]); g = blend_u8(gray_mean, g, f[1]); b = blend_u8(gray_mean, b, f[1]); }
        else if (op == 2) { const int l = gray_l(r, g, b); r = blend_u8(l, r, f[2]); g = blend_u8(l, g, f[2]); b = blend_u8(l, b, f[2]); }
        else if (op == 3) {
            int h, s, v;
            rgb2hsv_u8(r, g, b, h, s, v);
            h = (h + ((int)(f[3] * 255.0f) & 255)) & 255;
            hsv2rgb_u8(h, s, v, r, g, b);
        }
    }
}

// MODE 0: one workgroup per batch slot sums the gray level of its image as it is just before the contrast op -> gray_mean[slot]
// MODE 1: one thread per pixel applies all ops
template <int MODE>
__global__ __launch_bounds__(256) void jitter_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ idx,
                                                     const float* __restrict__ factors, const int32_t* __restrict__ order,
                                                     int32_t* __restrict__ gray_mean, uint8_t* __restrict__ dst, int n, int HW) {
    if (MODE == 0) {
        __shared__ unsigned long long part[256];
        const int slot = blockIdx.x;
        const float f[4] = {factors[slot * 4], factors[slot * 4 + 1], factors[slot * 4 + 2], factors[slot * 4 + 3]};
        const int ord[4] = {order[slot * 4], order[slot * 4 + 1], order[slot * 4 + 2], order[slot * 4 + 3]};
        const uint8_t* p = src + (size_t)idx[slot] * HW * 3;
        unsigned long long acc = 0;
        for (int i = threadIdx.x; i < HW; i += blockDim.x) {
            int r = p[i * 3], g = p[i * 3 + 1], b = p[i * 3 + 2];
            jitter_pixel(r, g, b, f, ord, 0, 1);                 // everything in front of the contrast op
            acc += (unsigned long long)gray_l(r, g, b);
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
            __syncthreads();
        }
        // ImageEnhance.Contrast: int(mean + 0.5) of the L image
        if (threadIdx.x == 0) gray_mean[slot] = (int)((2 * part[0] + (unsigned long long)HW) / (2ull * HW));
    } else {
        const size_t total = (size_t)n * HW;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
            const int slot = (int)(i / HW), px = (int)(i % HW);
            const float f[4] = {factors[slot * 4], factors[slot * 4 + 1], factors[slot * 4 + 2], factors[slot * 4 + 3]};
            const int ord[4] = {order[slot * 4], order[slot * 4 + 1], order[slot * 4 + 2], order[slot * 4 + 3]};
            const uint8_t* p = src + ((size_t)idx[slot] * HW + px) * 3;
            int r = p[0], g = p[1], b = p[2];
            jitter_pixel(r, g, b, f, ord, gray_mean[slot], 4);
            uint8_t* d = dst + i * 3;
            d[0] = (uint8_t)r; d[1] = (uint8_t)g; d[2] = (uint8_t)b;
        }
    }
}

// ColorJitter of a whole ragged image followed by crop / flip, without writing the jittered image: every op is pointwise once the
// contrast op's gray mean is known.  MODE 0 is jitter_kernel<0> over the slot's whole image (its own H x W); MODE 1 applies
// jitter_pixel only under the crop window, the padding stays 0 (RandomCrop pads after the jitter).
template <int MODE>
__global__ __launch_bounds__(256) void jitter_ragged_kernel(const uint8_t* __restrict__ arena, const long long* __restrict__ offsets,
                                                            const int32_t* __restrict__ sizes, long long n_src, const int32_t* __restrict__ params,
                                                            const float* __restrict__ factors, const int32_t* __restrict__ order,
                                                            int32_t* __restrict__ gray_mean, uint8_t* __restrict__ out, int bps, int Ho, int Wo,
                                                            int flip_first) {
    const int slot = MODE == 0 ? (int)blockIdx.x : (int)blockIdx.x / bps;
    const float f[4] = {factors[slot * 4], factors[slot * 4 + 1], factors[slot * 4 + 2], factors[slot * 4 + 3]};
    const int ord[4] = {order[slot * 4], order[slot * 4 + 1], order[slot * 4 + 2], order[slot * 4 + 3]};
    const RaggedImage im = ragged_image(arena, offsets, sizes, n_src, params[slot * 4]);
    if (MODE == 0) {
        __shared__ unsigned long long part[256];
        const size_t HW = im.base ? (size_t)im.H * im.W : 0;
        unsigned long long acc = 0;
        for (size_t i = threadIdx.x; i < HW; i += blockDim.x) {
            int r = im.base[i * 3], g = im.base[i * 3 + 1], b = im.base[i * 3 + 2];
            jitter_pixel(r, g, b, f, ord, 0, 1);                 // everything in front of the contrast op
            acc += (unsigned long long)gray_l(r, g, b);
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
            __syncthreads();
        }
        // ImageEnhance.Contrast: int(mean + 0.5) of the L image
        if (threadIdx.x == 0) gray_mean[slot] = HW ? (int)((2 * part[0] + (unsigned long long)HW) / (2ull * HW)) : 0;
    } else {
        const int partn = blockIdx.x % bps;
        const int top = params[slot * 4 + 1], left = params[slot * 4 + 2], flip = params[slot * 4 + 3];
        const int gm = gray_mean[slot];
        int s0, dir;
        ragged_columns(left, flip, flip_first, im.W, Wo, s0, dir);
        const int total = Ho * Wo;
        for (int i = partn * 256 + (int)threadIdx.x; i < total; i += bps * 256) {
            const int x = i % Wo, y = i / Wo;
            const int sy = top + y, sx = s0 + dir * x;
            int r = 0, g = 0, b = 0;
            if (im.base && sy >= 0 && sy < im.H && sx >= 0 && sx < im.W) {
                const uint8_t* p = im.base + ((size_t)sy * im.W + sx) * 3;
                r = p[0]; g = p[1]; b = p[2];
                jitter_pixel(r, g, b, f, ord, gm, 4);
            }
            uint8_t* o = out + ((size_t)slot * total + i) * 3;
            o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
        }
    }
}

}  // namespace

extern "C" int eoe_ragged_color_jitter_crop_u8(const uint8_t* arena, const int64_t* offsets, const int32_t* sizes, int64_t n_src,
                                               const int32_t* params, const float* factors, const int32_t* order,
                                               int32_t* gray_mean_scratch, uint8_t* out, int n, int Ho, int Wo, int flip_first, void* stream) {
    EOE_CHECK_ARG(n >= 0 && n_src > 0 && Ho > 0 && Wo > 0, "ragged_color_jitter_crop: bad args");
    if (n == 0) return 0;
    EOE_CHECK_ARG(arena && offsets && sizes && params && factors && order && gray_mean_scratch && out, "ragged_color_jitter_crop: bad args");
    EOE_CHECK_ARG((const void*)arena != (const void*)out, "ragged_color_jitter_crop: out must not alias the arena");
    EOE_CHECK_ARG(n < (1 << 22) && (size_t)Ho * Wo < (1u << 28), "ragged_color_jitter_crop: n < 2^22 and Ho*Wo < 2^28");
    const long long* off = reinterpret_cast<const long long*>(offsets);
    ProfScope ps("ragged_jitter_crop", 0, 3.0 * 2.0 * n * Ho * Wo, stream);
    hipLaunchKernelGGL(jitter_ragged_kernel<0>, dim3(n), dim3(256), 0, (hipStream_t)stream, arena, off, sizes, (long long)n_src, params, factors,
                       order, gray_mean_scratch, out, 1, Ho, Wo, flip_first);
    EOE_CHECK_LAUNCH("ragged_color_jitter_mean");
    const int bps = ragged_bps(n, (size_t)Ho * Wo);
    hipLaunchKernelGGL(jitter_ragged_kernel<1>, dim3((unsigned)((size_t)n * bps)), dim3(256), 0, (hipStream_t)stream, arena, off, sizes,
                       (long long)n_src, params, factors, order, gray_mean_scratch, out, bps, Ho, Wo, flip_first);
    EOE_CHECK_LAUNCH("ragged_color_jitter_crop");
    return 0;
}

extern "C" int eoe_ragged_resize_pass_u8(const uint8_t* src, uint8_t* dst, const int64_t* offs, const int32_t* desc, const int32_t* taps,
                                         int n, int64_t max_out_bytes, void* stream) {
    EOE_CHECK_ARG(n >= 0 && max_out_bytes >= 0, "ragged_resize_pass: bad args");
    if (n == 0 || max_out_bytes == 0) return 0;
    EOE_CHECK_ARG(src && dst && offs && desc && taps, "ragged_resize_pass: bad args");
    EOE_CHECK_ARG((const void*)src != (const void*)dst, "ragged_resize_pass: dst must not alias src");
    // workgroups per image: four output bytes per thread of the largest image, at most 64, and at most about 2^20 workgroups
    int64_t bpi = (max_out_bytes + 1023) / 1024;
    if (bpi > 64) bpi = 64;
    if (bpi * n > (1 << 20)) bpi = (1 << 20) / n;
    if (bpi < 1) bpi = 1;
    ProfScope ps("ragged_resize_pass", 0, 0.0, stream);
    hipLaunchKernelGGL(resize_pass_ragged_kernel, dim3((unsigned)((size_t)n * bpi)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       reinterpret_cast<const long long*>(offs), desc, taps, (int)bpi);
    EOE_CHECK_LAUNCH("ragged_resize_pass");
    return 0;
}

extern "C" int eoe_resize_coeffs(int in_size, int out_size, int filter, int32_t* bounds, int32_t* kk, int ksize_cap, int* ksize_out) {
    EOE_CHECK_ARG(in_size > 0 && out_size > 0 && (filter == EOE_RESIZE_BILINEAR || filter == EOE_RESIZE_BICUBIC),
                  "resize_coeffs: bad arguments");
    double (*fn)(double) = filter == EOE_RESIZE_BILINEAR ? filter_bilinear : filter_bicubic;
    const double support0 = filter == EOE_RESIZE_BILINEAR ? 1.0 : 2.0;
    const double scale = (double)in_size / (double)out_size;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = support0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (ksize_out) *ksize_out = ksize;
    if (!bounds || !kk) return 0;                       // size query
    EOE_CHECK_ARG(ksize_cap >= ksize, "resize_coeffs: kk holds %d taps per output, %d needed", ksize_cap, ksize);
    const double ss = 1.0 / filterscale;
    double* w = (double*)malloc(sizeof(double) * ksize);
    if (!w) return eoe_set_error(EOE_ERR_LAUNCH, "resize_coeffs: out of memory");
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) { w[x] = fn((x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            kk[(size_t)xx * ksize_cap + x] = w[x] < 0 ? (int32_t)(-0.5 + w[x] * (1 << RESIZE_PRECISION_BITS))
                                                      : (int32_t)(0.5 + w[x] * (1 << RESIZE_PRECISION_BITS));
        }
        for (int x = xmax; x < ksize_cap; ++x) kk[(size_t)xx * ksize_cap + x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    free(w);
    return 0;
}

extern "C" int eoe_resize_pass_u8(const uint8_t* src, uint8_t* dst, const int32_t* bounds, const int32_t* kk, int ksize, int64_t outer,
                                  int axis_in, int axis_out, int inner, void* stream) {
    EOE_CHECK_ARG(src && dst && bounds && kk && ksize > 0 && outer > 0 && axis_in > 0 && axis_out > 0 && inner > 0, "resize_pass: bad args");
    const size_t total = (size_t)outer * axis_out * inner;
    ProfScope ps("resize_pass", 0, (double)outer * axis_in * inner + (double)total, stream);
    size_t g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(resize_pass_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, dst, bounds, kk, ksize, (size_t)outer,
                       axis_in, axis_out, inner);
    EOE_CHECK_LAUNCH("resize_pass");
    return 0;
}

extern "C" int eoe_color_jitter_u8(const uint8_t* src, int64_t n_src, const int32_t* idx, const float* factors, const int32_t* order,
                                   int32_t* gray_mean_scratch, uint8_t* dst, int n, int H, int W, void* stream) {
    EOE_CHECK_ARG(src && idx && factors && order && gray_mean_scratch && dst && n_src > 0 && n > 0 && H > 0 && W > 0 &&
                  (size_t)H * W < (1u << 30), "color_jitter: bad args");
    ProfScope ps("color_jitter", 0, 3.0 * 3.0 * n * H * W, stream);
    hipLaunchKernelGGL(jitter_kernel<0>, dim3(n), dim3(256), 0, (hipStream_t)stream, src, idx, factors, order, gray_mean_scratch, dst, n, H * W);
    EOE_CHECK_LAUNCH("color_jitter_mean");
    size_t g = ((size_t)n * H * W + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(jitter_kernel<1>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, idx, factors, order, gray_mean_scratch, dst, n,
                       H * W);
    EOE_CHECK_LAUNCH("color_jitter_apply");
    return 0;
}
