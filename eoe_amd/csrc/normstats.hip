// Per-task input normalisation: what the reference's dataset base class makes of the strings 'normalize' / 'gcn-normalize'
// (`datasets/bases.py:293-372`) and the per-sample operator its GCN mode leaves on the step path
// (`utils/transformations.py:326-349` GlobalContrastNormalization followed by a per-channel Normalize).
//
// eoe_set_moments_u8: the statistics pass over a resident uint8 NHWC image set, one launch, one workgroup per listed image.
//   Everything is an exact integer: per channel sum(v) and sum(v^2), per image min, max and sum |N v - S| (N = C*H*W features,
//   S = sum(v) over the image), i.e. the image's L1 deviation from its mean times 255 N.  Integer sums do not depend on the
//   reduction tree, so the results are bitwise repeatable and identical on every rank; the host (eoe_amd/normalize.py) turns them
//   into the reference's RunningStats recurrence / GCN extremes in float64.  Two passes over the image (S first), the second from
//   L2 (an image of the set is at most a few hundred KB).
//
// eoe_gcn_normalize: y = ((x - mean_i) / scale_i - shift[c]) / range[c] on fp32 NCHW, per sample i with mean_i over all N features
//   and scale_i = mean |x - mean_i| (l1) or sqrt(sum (x - mean_i)^2) / N (l2, the reference's definition).  One workgroup per
//   sample, so a sample's passes stay on one XCD: sum -> mean, deviation -> scale, write.  Each thread keeps its first R chunks
//   in registers across the three passes and re-reads only the rest:
//     * N <= 4096 (3 x 32 x 32, 1 x 28 x 28): 256 threads x 4 float4 -- the whole sample in registers, one pass over memory;
//     * larger (3 x 224 x 224 = 602 KB, more than the LDS holds): 1024 threads x 12 float4 = 192 KB in registers (16 chunks per
//       thread spill under the 128-register budget of a 1024-thread workgroup), the other 410 KB come back from L2 / Infinity
//       Cache twice.
//     * a feature count that is no multiple of 4, or an x / y that is not 16-byte aligned, takes a fallback: the same kernel with
//       scalar loads and 256 threads per sample whatever its size.  Correct (tested at 3 x 5 x 7), but slow for large samples
//       (3 x 225 x 225 would run many times slower than 3 x 224 x 224); every shape of the reference's runners is a multiple of 4.
//   The sums and the final affine run in fp64 (the kernel is memory-bound; this keeps it at the rounding of the output alone),
//   in a fixed order: per thread in chunk order, xor butterfly inside a wave, waves in index order.  No atomics.  No epsilon: a
//   constant image gives non-finite values, as in the reference.  In place (y == x) is allowed: every element is read and written
//   by the same thread, so the result equals the out-of-place one bit for bit.
#include "common.h"
#include <math.h>

namespace {

constexpr int MOM_NT = 256;
constexpr long long MAX_FEATURES = 1ll << 26;      // N^2 * 255 stays far inside int64

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workgroup sum of K values per thread; every thread gets the totals.  red: K * (NT / 64) words
template <int NT, int K>
__device__ void block_sum_u64(unsigned long long (&v)[K], unsigned long long* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                           // red may still be read from an earlier call
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long s = wave_sum_u64(v[k]);
        if (lane == 0) red[k * (NT / 64) + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned long long s = 0;
        for (int w = 0; w < NT / 64; ++w) s += red[k * (NT / 64) + w];
        v[k] = s;
    }
}

template <int NT>
__device__ double block_sum_f64(double v, double* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_sum_f64(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ unsigned byte_of(const u32x4& u, int k) { return (u[k >> 2] >> ((k & 3) * 8)) & 0xffu; }

// ---- eoe_set_moments_u8 ---------------------------------------------------------------------------------------------------
// chan: [n_index][C][2] = (sum v, sum v^2); img: [n_index][3] = (min, max, sum |N v - S|).  An index outside the set writes -1
// everywhere for that image and reads nothing.
__global__ __launch_bounds__(MOM_NT) void moments_kernel(const uint8_t* __restrict__ src, long long n_src, int N, int C,
                                                         const long long* __restrict__ index, long long* __restrict__ chan,
                                                         long long* __restrict__ img, int vec16) {
    __shared__ unsigned long long red[8 * (MOM_NT / 64)];
    const int t = threadIdx.x;
    const long long b = blockIdx.x, row = index ? index[b] : b;
    if (row < 0 || row >= n_src) {                             // uniform over the workgroup
        if (t < 2 * C) chan[b * 2 * C + t] = -1;
        if (t < 3) img[b * 3 + t] = -1;
        return;
    }
    const uint8_t* p = src + (size_t)row * N;
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};            // per channel: sum v (0..2), sum v^2 (3..5)
    unsigned mn = 255u, mx = 0u;
    if (vec16) {
        const u32x4* pv = reinterpret_cast<const u32x4*>(p);
        for (int i = t; i < N / 16; i += MOM_NT) {
            const u32x4 u = pv[i];
            unsigned ls[3] = {0, 0, 0}, lq[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned v = byte_of(u, k);
                ls[k % 3] += v;
                lq[k % 3] += v * v;
                mn = min(mn, v);
                mx = max(mx, v);
            }
            // byte 16 i + k has channel (i + k) % 3 (16 = 1 mod 3): rotate the local slots by the chunk's phase
            const int ph = (C == 3) ? i % 3 : 0;
            if (C == 1) {
                acc[0] += ls[0] + ls[1] + ls[2];
                acc[3] += lq[0] + lq[1] + lq[2];
            } else if (ph == 0) {
                acc[0] += ls[0]; acc[1] += ls[1]; acc[2] += ls[2]; acc[3] += lq[0]; acc[4] += lq[1]; acc[5] += lq[2];
            } else if (ph == 1) {
                acc[1] += ls[0]; acc[2] += ls[1]; acc[0] += ls[2]; acc[4] += lq[0]; acc[5] += lq[1]; acc[3] += lq[2];
            } else {
                acc[2] += ls[0]; acc[0] += ls[1]; acc[1] += ls[2]; acc[5] += lq[0]; acc[3] += lq[1]; acc[4] += lq[2];
            }
        }
    } else {
        for (int j = t; j < N; j += MOM_NT) {
            const unsigned v = p[j];
            const int c = (C == 3) ? j % 3 : 0;
            mn = min(mn, v);
            mx = max(mx, v);
            if (c == 0) { acc[0] += v; acc[3] += v * v; }
            else if (c == 1) { acc[1] += v; acc[4] += v * v; }
            else { acc[2] += v; acc[5] += v * v; }
        }
    }
    // min / max: butterfly inside the wave, the waves' values through LDS
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (unsigned)__shfl_xor((int)mn, o, 64));
        mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
    }
    __shared__ unsigned mm[2 * (MOM_NT / 64)];
    if ((t & 63) == 0) { mm[t >> 6] = mn; mm[MOM_NT / 64 + (t >> 6)] = mx; }
    unsigned long long sums[6] = {acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]};
    block_sum_u64<MOM_NT, 6>(sums, red);                       // its barriers also publish mm
    for (int w = 0; w < MOM_NT / 64; ++w) { mn = min(mn, mm[w]); mx = max(mx, mm[MOM_NT / 64 + w]); }
    const long long S = (long long)(sums[0] + sums[1] + sums[2]);
    // second pass: sum |N v - S|
    unsigned long long dev[1] = {0};
    if (vec16) {
        const u32x4* pv = reinterpret_cast<const u32x4*>(p);
        for (int i = t; i < N / 16; i += MOM_NT) {
            const u32x4 u = pv[i];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long d = (long long)N * (long long)byte_of(u, k) - S;
                dev[0] += (unsigned long long)(d < 0 ? -d : d);
            }
        }
    } else {
        for (int j = t; j < N; j += MOM_NT) {
            const long long d = (long long)N * (long long)p[j] - S;
            dev[0] += (unsigned long long)(d < 0 ? -d : d);
        }
    }
    block_sum_u64<MOM_NT, 1>(dev, red);
    if (t == 0) {
        for (int c = 0; c < C; ++c) {
            chan[(b * C + c) * 2 + 0] = (long long)sums[c];
            chan[(b * C + c) * 2 + 1] = (long long)sums[3 + c];
        }
        img[b * 3 + 0] = mn;
        img[b * 3 + 1] = mx;
        img[b * 3 + 2] = (long long)dev[0];
    }
}

// ---- eoe_gcn_normalize ----------------------------------------------------------------------------------------------------
template <int V> __device__ __forceinline__ void load_chunk(const float* p, float (&o)[V]) {
    if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    } else {
        o[0] = *p;
    }
}
template <int V> __device__ __forceinline__ void store_chunk(float* p, const float (&o)[V]) {
    if constexpr (V == 4) {
        f32x4 v;
        v[0] = o[0]; v[1] = o[1]; v[2] = o[2]; v[3] = o[3];
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        *p = o[0];
    }
}

// The cached chunks live as 32-bit floats between the passes: without this the compiler keeps their fp64 conversions of one pass
// alive for the next (2 registers per value) and spills.  An empty statement that claims to modify each register.
template <int R, int V> __device__ __forceinline__ void pin_regs(float (&reg)[R][V]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < V; ++k) asm volatile("" : "+v"(reg[r][k]));
}

struct GcnCoef { double a0, a1, a2, b0, b1, b2; int HW, HW2; };

template <int V> __device__ __forceinline__ void emit_chunk(float* ys, int ch, const float (&v)[V], const GcnCoef k) {
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = ch * V + j;
        const double a = e < k.HW ? k.a0 : (e < k.HW2 ? k.a1 : k.a2), b = e < k.HW ? k.b0 : (e < k.HW2 ? k.b1 : k.b2);
        o[j] = (float)fma((double)v[j], a, b);
    }
    store_chunk<V>(ys + (size_t)ch * V, o);
}

// NT threads per sample, chunks of V floats, the first R chunks of every thread kept in registers
template <int NT, int R, int V>
__global__ __launch_bounds__(NT) void gcn_kernel(const float* x, float* y, int N, int HW, int C, int l2, const float* shift,
                                                 const float* range) {      // no __restrict__: y may be x
    __shared__ double red1[NT / 64], red2[NT / 64];
    const int t = threadIdx.x, nchunks = N / V;
    const float* xs = x + (size_t)blockIdx.x * N;
    float* ys = y + (size_t)blockIdx.x * N;
    float reg[R][V];
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ch = t + r * NT;
        if (ch < nchunks) {
            load_chunk<V>(xs + (size_t)ch * V, reg[r]);
#pragma unroll
            for (int k = 0; k < V; ++k) s += (double)reg[r][k];
        }
    }
    for (int ch = t + R * NT; ch < nchunks; ch += NT) {
        float v[V];
        load_chunk<V>(xs + (size_t)ch * V, v);
#pragma unroll
        for (int k = 0; k < V; ++k) s += (double)v[k];
    }
    const double mean = block_sum_f64<NT>(s, red1) / (double)N;
    pin_regs<R, V>(reg);
    double dsum = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (t + r * NT < nchunks) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const double d = (double)reg[r][k] - mean;
                dsum += l2 ? d * d : fabs(d);
            }
        }
    }
    for (int ch = t + R * NT; ch < nchunks; ch += NT) {
        float v[V];
        load_chunk<V>(xs + (size_t)ch * V, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double d = (double)v[k] - mean;
            dsum += l2 ? d * d : fabs(d);
        }
    }
    dsum = block_sum_f64<NT>(dsum, red2);
    pin_regs<R, V>(reg);
    const double scale = l2 ? sqrt(dsum) / (double)N : dsum / (double)N;
    // y = x * a[c] + b[c]
    GcnCoef k;
    k.HW = HW;
    k.HW2 = 2 * HW;
    {
        const double sh0 = shift ? (double)shift[0] : 0.0, rg0 = range ? (double)range[0] : 1.0;
        const double sh1 = (shift && C > 1) ? (double)shift[1] : 0.0, rg1 = (range && C > 1) ? (double)range[1] : 1.0;
        const double sh2 = (shift && C > 2) ? (double)shift[2] : 0.0, rg2 = (range && C > 2) ? (double)range[2] : 1.0;
        const double ms = mean / scale;
        k.a0 = 1.0 / (scale * rg0); k.b0 = -(ms + sh0) / rg0;
        k.a1 = 1.0 / (scale * rg1); k.b1 = -(ms + sh1) / rg1;
        k.a2 = 1.0 / (scale * rg2); k.b2 = -(ms + sh2) / rg2;
    }
    // the streamed chunks first; in place, a thread only ever overwrites chunks it alone reads
    for (int ch = t + R * NT; ch < nchunks; ch += NT) {
        float v[V];
        load_chunk<V>(xs + (size_t)ch * V, v);
        emit_chunk<V>(ys, ch, v, k);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ch = t + r * NT;
        if (ch < nchunks) emit_chunk<V>(ys, ch, reg[r], k);
    }
}

}  // namespace

extern "C" int eoe_set_moments_u8(const uint8_t* src, int64_t n_src, int H, int W, int C, const int64_t* index, int64_t n_index,
                                  int64_t* chan_sums, int64_t* img_stats, void* stream) {
    EOE_CHECK_ARG(src && chan_sums && img_stats, "set_moments_u8: null image set or output");
    EOE_CHECK_ARG(C == 1 || C == 3, "set_moments_u8: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(n_src > 0 && H > 0 && W > 0, "set_moments_u8: n_src, H and W must be positive");
    EOE_CHECK_ARG((long long)H * W * C <= MAX_FEATURES, "set_moments_u8: images of at most %lld values (%d x %d x %d)", MAX_FEATURES, H, W, C);
    EOE_CHECK_ARG(n_index > 0 && n_index < (1ll << 31), "set_moments_u8: n_index must be in [1, 2^31), not %lld", (long long)n_index);
    const int N = H * W * C;
    const int vec16 = (N % 16 == 0) && (((uintptr_t)src & 15) == 0);
    ProfScope ps("set_moments_u8", 0, 2.0 * (double)N * (double)n_index, stream);
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)n_index), dim3(MOM_NT), 0, (hipStream_t)stream, src, (long long)n_src, N, C,
                       (const long long*)index, (long long*)chan_sums, (long long*)img_stats, vec16);
    EOE_CHECK_LAUNCH("set_moments_u8");
    return 0;
}

extern "C" int eoe_gcn_normalize(const float* x, float* y, int n, int C, int H, int W, int scale, const float* shift, const float* range,
                                 void* stream) {
    EOE_CHECK_ARG(x && y, "gcn_normalize: null input or output");
    EOE_CHECK_ARG(C == 1 || C == 3, "gcn_normalize: C must be 1 or 3, not %d", C);
    EOE_CHECK_ARG(n > 0 && H > 0 && W > 0, "gcn_normalize: n, H and W must be positive");
    EOE_CHECK_ARG(scale == EOE_GCN_L1 || scale == EOE_GCN_L2, "gcn_normalize: unknown scale %d (EOE_GCN_L1 = 1, EOE_GCN_L2 = 2)", scale);
    EOE_CHECK_ARG((shift == nullptr) == (range == nullptr), "gcn_normalize: shift and range go together (both or neither)");
    EOE_CHECK_ARG((long long)H * W * C <= MAX_FEATURES, "gcn_normalize: samples of at most %lld values (%d x %d x %d)", MAX_FEATURES, C, H, W);
    const int HW = H * W, N = C * HW, l2 = scale == EOE_GCN_L2;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (N % 4 == 0) && ((((uintptr_t)x | (uintptr_t)y) & 15) == 0);
    ProfScope ps("gcn_normalize", 6.0 * (double)N * n, 8.0 * (double)N * n, stream);
    if (vec && N <= 256 * 4 * 4)
        hipLaunchKernelGGL((gcn_kernel<256, 4, 4>), dim3((unsigned)n), dim3(256), 0, st, x, y, N, HW, C, l2, shift, range);
    else if (vec)
        hipLaunchKernelGGL((gcn_kernel<1024, 12, 4>), dim3((unsigned)n), dim3(1024), 0, st, x, y, N, HW, C, l2, shift, range);
    else
        hipLaunchKernelGGL((gcn_kernel<256, 16, 1>), dim3((unsigned)n), dim3(256), 0, st, x, y, N, HW, C, l2, shift, range);
    EOE_CHECK_LAUNCH("gcn_normalize");
    return 0;
}
