// Attention rollout (Abnar & Zuidema 2020) for the ViT towers: where the class token's attention comes from, from the forward pass alone.
//   eoe_attn_probs    the softmax probabilities the attention kernels keep in registers, fused over the heads: probs fp32 [n, L, L] from the
//                     packed 16-bit q | k | v of eoe_attn_fwd, 1 <= L <= EOE_ATTN_LONG_MAX_L.  One workgroup of four wavefronts per (image,
//                     strip of 16 queries), the heads in a loop inside.  Per head: S^T = K Q^T on the matrix cores (attn_frag.h: key on the
//                     accumulator row, query on the lane; wave w takes the 16-key tiles w, w + 4, ..., its operands straight from global memory
//                     through the bounds-checked buffer resource, every K row is used once per strip), the scaled scores of the strip go to
//                     LDS (16 x 656 fp32, 41 KB: three workgroups per CU), 16 lanes per query take the fp32 softmax with the row maximum
//                     subtracted, and each lane folds its columns (16 i + lane & 15) into 40 accumulator registers: sum / max / min over the
//                     heads in head order.  Keys >= L are never stored, read or written (the short kernel's -inf mask); query rows >= L are
//                     computed from zeros and dropped.  The finished strip -- 16 consecutive rows of probs, one contiguous range -- goes
//                     back through LDS and is written once, coalesced.  The V third is never read.
//   eoe_rollout_step  r_out = A^ r_in per image in fp32, A^ = row-normalised ((1 - residual) probs + residual I) formed while the A tile is
//                     staged (never written to memory): a 64 x 64 x 16 LDS-tiled fp32 FMA product, 4 x 4 outputs per lane, k ascending.  The
//                     row sums of a workgroup's 64 rows are taken first: a wavefront per row, lanes stride the columns in order, xor-shuffle
//                     tree; a sum within 2^-20 of one (its own rounding) counts as one, so a normalised row keeps its bits.  r_in == NULL runs the same kernel with the B tile generated (k == j) instead of loaded: the same operations on the
//                     same values as an explicit identity, so the same bits.
//   eoe_rollout_map   the class token's row of r without its class column, every patch block constant: maps fp32 [n, grid patch, grid patch].
// No atomics, nothing allocated; every output element is written by one lane after loops in a fixed order: two runs give the same bits.
#include <math.h>

#include "attn_frag.h"

namespace {

using namespace attn_frag;

constexpr int RO_NT = 256;
constexpr int RO_QS = 16;                                   // queries per strip = one MFMA tile
constexpr int RO_LP = 656;                                  // LDS row pitch in floats: >= 640, 16-byte rows, 16 banks from row to row
constexpr int RO_PER = EOE_ATTN_LONG_MAX_L / 16;            // columns per lane of a 16-lane row group
static_assert(EOE_ATTN_LONG_MAX_L % 16 == 0 && RO_LP >= EOE_ATTN_LONG_MAX_L && RO_LP % 4 == 0, "strip layout");

enum { FUSE_MEAN = EOE_FUSE_MEAN, FUSE_MAX = EOE_FUSE_MAX, FUSE_MIN = EOE_FUSE_MIN };

__device__ __forceinline__ float row16_max(float v) {       // over the 16 lanes sharing lane >> 4
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    v = fmaxf(v, __shfl_xor(v, 4, 64));
    return fmaxf(v, __shfl_xor(v, 8, 64));
}
__device__ __forceinline__ float row16_add(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v + __shfl_xor(v, 8, 64);
}

// ------------------------------------------------------------------------------------------------ probabilities
template <typename T>
__global__ __launch_bounds__(RO_NT) void attn_probs_kernel(const T* __restrict__ qkv, float* __restrict__ probs, int L, int heads, int nstrips,
                                                           int fuse, float inv_heads) {
    __shared__ __attribute__((aligned(16))) float sc[RO_QS * RO_LP];
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int strip = (int)(blockIdx.x % (unsigned)nstrips), img = (int)(blockIdx.x / (unsigned)nstrips);
    const int q0 = strip * RO_QS;
    const int D = heads * 64, ld = 3 * D;
    const unsigned pitchb = (unsigned)ld * 2u, kcb = (unsigned)D * 2u;
    const int ntiles = (L + 15) >> 4;
    const int row = tid >> 4, sub = tid & 15;               // the softmax: 16 lanes per query, lane `sub` owns columns sub + 16 i
    float* my = sc + row * RO_LP;
    float acc[RO_PER];
#pragma unroll
    for (int i = 0; i < RO_PER; ++i) acc[i] = 0.f;

    for (int h = 0; h < heads; ++h) {
        const T* base = qkv + (size_t)img * L * ld + h * 64;
        const __amdgpu_buffer_rsrc_t rq = qkv_rsrc(base, L, ld, D);
        V8<T> qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[ks] = rowfrag<T>(rq, pitchb, 0u, L, q0 + lr, ks, lane);
        for (int t = w; t < ntiles; t += 4) {
            f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) s = T16<T>::mfma16(bfrag<T>(rq, pitchb, kcb, L, t, ks, lane), qf[ks], s);
            // register r of lane (lr, lg) = key 16 t + 4 lg + r of query q0 + lr
            *(f32x4*)(sc + lr * RO_LP + 16 * t + 4 * lg) = s * 0.125f;           // 1 / sqrt(64)
        }
        __syncthreads();
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < RO_PER; ++i) {
            const int c = sub + 16 * i;
            if (c < L) m = fmaxf(m, my[c]);
        }
        m = row16_max(m);                                   // finite: key 0 < L
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < RO_PER; ++i) {
            const int c = sub + 16 * i;
            if (c < L) {
                const float e = expf(my[c] - m);
                my[c] = e;                                  // this lane's own element: no barrier between the passes
                sum += e;
            }
        }
        sum = row16_add(sum);
#pragma unroll
        for (int i = 0; i < RO_PER; ++i) {
            const int c = sub + 16 * i;
            if (c < L) {
                const float p = my[c] / sum;
                acc[i] = h == 0 ? p : fuse == FUSE_MEAN ? acc[i] + p : fuse == FUSE_MAX ? fmaxf(acc[i], p) : fminf(acc[i], p);
            }
        }
        __syncthreads();                                    // the next head's scores overwrite the strip
    }
#pragma unroll
    for (int i = 0; i < RO_PER; ++i) {
        const int c = sub + 16 * i;
        if (c < L) my[c] = fuse == FUSE_MEAN ? acc[i] * inv_heads : acc[i];
    }
    __syncthreads();
    // rows q0 .. q0 + valid - 1 of this image's [L, L] matrix are one contiguous range
    const int valid = min(RO_QS, L - q0);
    float* out = probs + ((size_t)img * L + q0) * L;
    for (int e = tid; e < valid * L; e += RO_NT) {
        const int r = e / L;
        out[e] = sc[r * RO_LP + (e - r * L)];
    }
}

// ------------------------------------------------------------------------------------------------ one rollout step
constexpr int RS_BM = 64, RS_BN = 64, RS_BK = 16, RS_PAD = 4;
// The worst-case rounding of a row sum near one in this kernel's order at L = 640: 10 additions per lane and 6 tree levels of 2^-24 each.
// A sum that close to one says nothing against "this row sums to one"; dividing by it would move last bits and normalise nothing.
constexpr float RS_ONE_TOL = 0x1p-20f;
static_assert((EOE_ATTN_LONG_MAX_L + 63) / 64 + 6 <= 16, "RS_ONE_TOL covers the row sum's own rounding");

template <bool IDENT>
__global__ __launch_bounds__(256) void rollout_step_kernel(const float* __restrict__ probs, const float* __restrict__ rin, float* __restrict__ rout,
                                                           int L, float residual) {
    __shared__ __attribute__((aligned(16))) float As[RS_BK][RS_BM + RS_PAD];      // [k][row]
    __shared__ __attribute__((aligned(16))) float Bs[RS_BK][RS_BN + RS_PAD];      // [k][column]
    __shared__ float rsum[RS_BM];                           // the row's divisor; 0: the identity row
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m0 = blockIdx.y * RS_BM, n0 = blockIdx.x * RS_BN;
    const size_t img = blockIdx.z;
    const float* P = probs + img * L * L;
    const float* R = IDENT ? nullptr : rin + img * L * L;
    float* O = rout + img * L * L;
    const float keep = 1.0f - residual;

    // the sums of A^'s rows m0 .. m0 + 63 before the division: wave w takes rows 16 w .. 16 w + 15, one after the other
    for (int r = 16 * w; r < 16 * w + 16; ++r) {
        const int gm = m0 + r;
        float s = 0.f;
        if (gm < L)
            for (int c = lane; c < L; c += 64) s += keep * P[(size_t)gm * L + c] + (c == gm ? residual : 0.f);
        s = wave_sum(s);
        // 0, inf, NaN -> identity row.  A sum within RS_ONE_TOL of one IS one: the difference is no more than this sum's own rounding,
        // so a row that is already normalised (a softmax row, the mean of softmax rows) keeps its bits instead of gaining a rounding
        if (lane == 0) rsum[r] = !(s != 0.f && fabsf(s) < INFINITY) ? 0.f : fabsf(s - 1.0f) <= RS_ONE_TOL ? 1.0f : s;
    }
    __syncthreads();

    const int tx = tid & 15, ty = tid >> 4;                 // outputs: rows 4 ty .. + 3, columns 4 tx .. + 3
    const int ar = tid >> 2, ak = (tid & 3) * 4;            // staging A: row ar, k ak .. ak + 3
    const int bk = tid >> 4, bc = (tid & 15) * 4;           // staging B: k bk, columns bc .. bc + 3
    const int gm = m0 + ar;
    const float div = rsum[ar];
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int k0 = 0; k0 < L; k0 += RS_BK) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gk = k0 + ak + j;
            float a = 0.f;
            if (gm < L && gk < L)
                a = div != 0.f ? (keep * P[(size_t)gm * L + gk] + (gk == gm ? residual : 0.f)) / div : (gk == gm ? 1.f : 0.f);
            As[ak + j][ar] = a;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gk = k0 + bk, gc = n0 + bc + j;
            float b = 0.f;
            if (gk < L && gc < L) b = IDENT ? (gk == gc ? 1.f : 0.f) : R[(size_t)gk * L + gc];
            Bs[bk][bc + j] = b;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < RS_BK; ++kk) {
            const f32x4 a = *(const f32x4*)&As[kk][4 * ty];
            const f32x4 b = *(const f32x4*)&Bs[kk][4 * tx];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int om = m0 + 4 * ty + i;
        if (om >= L) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oc = n0 + 4 * tx + j;
            if (oc < L) O[(size_t)om * L + oc] = acc[i][j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ the map
__global__ __launch_bounds__(RO_NT) void rollout_map_kernel(const float* __restrict__ r, float* __restrict__ maps, unsigned total, int L, int grid,
                                                            FDiv plane_d, FDiv res_d, FDiv patch_d) {
    const unsigned e = blockIdx.x * RO_NT + threadIdx.x;
    if (e >= total) return;
    unsigned img, pix, y, x;
    plane_d.divmod(e, img, pix);
    res_d.divmod(pix, y, x);
    maps[e] = r[(size_t)img * L * L + 1u + patch_d.div(y) * (unsigned)grid + patch_d.div(x)];
}

inline bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" int eoe_attn_probs(const void* qkv, float* probs, int n, int L, int heads, int dtype, int fuse, void* stream) {
    EOE_CHECK_ARG(qkv && probs, "attn_probs: null qkv or probs");
    EOE_CHECK_ARG(n > 0, "attn_probs: n must be positive, not %d", n);
    EOE_CHECK_ARG(L >= 1 && L <= EOE_ATTN_LONG_MAX_L, "attn_probs: sequence length %d not in [1, %d]", L, EOE_ATTN_LONG_MAX_L);
    EOE_CHECK_ARG(heads > 0 && heads <= 4096, "attn_probs: heads must be in [1, 4096], not %d", heads);
    EOE_CHECK_ARG(dtype == EOE_F16 || dtype == EOE_BF16, "attn_probs: bad dtype %d", dtype);
    EOE_CHECK_ARG(fuse == FUSE_MEAN || fuse == FUSE_MAX || fuse == FUSE_MIN, "attn_probs: fuse %d is none of EOE_FUSE_*", fuse);
    EOE_CHECK_ARG(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)probs & 3) == 0, "attn_probs: qkv must be 16-byte and probs 4-byte aligned");
    const int nstrips = (L + RO_QS - 1) / RO_QS;
    EOE_CHECK_ARG((double)n * nstrips < 2147483647.0, "attn_probs: too many workgroups");
    const float inv_heads = 1.0f / (float)heads;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("attn_probs", 2.0 * n * heads * (double)L * L * 64, (double)n * L * (4.0 * heads * 64 + 4.0 * L), stream);
    if (dtype == EOE_F16)
        hipLaunchKernelGGL((attn_probs_kernel<f16_t>), dim3((unsigned)(n * nstrips)), dim3(RO_NT), 0, st, (const f16_t*)qkv, probs, L, heads, nstrips,
                           fuse, inv_heads);
    else
        hipLaunchKernelGGL((attn_probs_kernel<bf16_t>), dim3((unsigned)(n * nstrips)), dim3(RO_NT), 0, st, (const bf16_t*)qkv, probs, L, heads,
                           nstrips, fuse, inv_heads);
    EOE_CHECK_LAUNCH("attn_probs");
    return 0;
}

extern "C" int eoe_rollout_step(const float* probs, const float* r_in, float* r_out, int n, int L, float residual, void* stream) {
    EOE_CHECK_ARG(probs && r_out, "rollout_step: null probs or r_out");
    EOE_CHECK_ARG(n > 0 && n <= 65535, "rollout_step: n must be in [1, 65535], not %d", n);
    EOE_CHECK_ARG(L >= 1 && L <= EOE_ATTN_LONG_MAX_L, "rollout_step: sequence length %d not in [1, %d]", L, EOE_ATTN_LONG_MAX_L);
    EOE_CHECK_ARG(residual >= 0.0f && residual < 1.0f, "rollout_step: residual must be in [0, 1), not %g", (double)residual);
    const size_t bytes = (size_t)n * L * L * 4;
    EOE_CHECK_ARG(!r_in || !overlap(r_out, r_in, bytes), "rollout_step: r_out must not alias r_in");
    EOE_CHECK_ARG(!overlap(r_out, probs, bytes), "rollout_step: r_out must not alias probs");
    EOE_CHECK_ARG((((uintptr_t)probs | (uintptr_t)r_in | (uintptr_t)r_out) & 3) == 0, "rollout_step: probs, r_in and r_out must be 4-byte aligned");
    const dim3 grid((unsigned)cdiv(L, RS_BN), (unsigned)cdiv(L, RS_BM), (unsigned)n);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("rollout_step", 2.0 * n * (double)L * L * L, 12.0 * n * (double)L * L, stream);
    if (r_in) hipLaunchKernelGGL(rollout_step_kernel<false>, grid, dim3(256), 0, st, probs, r_in, r_out, L, residual);
    else hipLaunchKernelGGL(rollout_step_kernel<true>, grid, dim3(256), 0, st, probs, r_in, r_out, L, residual);
    EOE_CHECK_LAUNCH("rollout_step");
    return 0;
}

extern "C" int eoe_rollout_map(const float* r, float* maps, int n, int L, int grid, int patch, void* stream) {
    EOE_CHECK_ARG(r && maps, "rollout_map: null r or maps");
    EOE_CHECK_ARG(n > 0, "rollout_map: n must be positive, not %d", n);
    EOE_CHECK_ARG(L >= 1 && L <= EOE_ATTN_LONG_MAX_L, "rollout_map: sequence length %d not in [1, %d]", L, EOE_ATTN_LONG_MAX_L);
    EOE_CHECK_ARG(grid >= 1 && grid <= 25 && L == grid * grid + 1, "rollout_map: L = %d is not grid^2 + 1 (grid = %d)", L, grid);
    EOE_CHECK_ARG(patch >= 1 && patch <= 1024, "rollout_map: patch must be in [1, 1024], not %d", patch);
    EOE_CHECK_ARG((((uintptr_t)r | (uintptr_t)maps) & 3) == 0, "rollout_map: r and maps must be 4-byte aligned");
    const long long res = (long long)grid * patch, total = (long long)n * res * res;
    EOE_CHECK_ARG(total < (1ll << 31), "rollout_map: n * (grid * patch)^2 = %lld pixels exceed 32-bit indexing", total);
    ProfScope ps("rollout_map", 0.0, 4.0 * (double)total + 4.0 * n * (double)(L - 1), stream);
    hipLaunchKernelGGL(rollout_map_kernel, dim3((unsigned)((total + RO_NT - 1) / RO_NT)), dim3(RO_NT), 0, (hipStream_t)stream, r, maps,
                       (unsigned)total, L, grid, FDiv((unsigned)(res * res)), FDiv((unsigned)res), FDiv((unsigned)patch));
    EOE_CHECK_LAUNCH("rollout_map");
    return 0;
}
