// The fp32 tile layer of the feature-space kernels (knn.hip, mahalanobis.hip): a 128 x 128 tile of C[a][b] = sum_k A[a][k] B[b][k] on
// v_mfma_f32_32x32x2_f32 -- fp32 in, fp32 accumulate, bit for bit a k-ordered fmaf chain, so no 16-bit rounding enters a ranking.
//
//   workgroup     256 threads = 4 waves as 2 x 2.  Wave (wa, wb) owns rows [64 wa, 64 wa + 64) of A times rows [64 wb, 64 wb + 64) of B:
//                 2 x 2 MFMA tiles of 32 x 32, 64 accumulator registers per lane.  From one wave per SIMD the four independent
//                 accumulators already reach the fp32 MFMA rate.
//   operand image k-major, [32][LD] floats per operand and k-step: element (k, row) of the step lies at k * LD + row, row = 0 .. 127.
//                 An MFMA operand read is then 32 consecutive floats per half wave (lanes 0-31 read k, lanes 32-63 read k + 1).
//                 LD = 129 (LD_QUAD) for an operand whose rows run along k in memory: a 16-byte global load holds four k of ONE row
//                 and goes to LDS as four element stores (store_quad_t); the odd stride spreads them over the banks.
//                 LD = 160 (LD_ROWS) for an operand that lies k-major in memory already: its rows go to LDS as 16-byte stores, and
//                 160 = 32 mod 64 puts the two half waves of an operand read on the two halves of the 64 banks.
//                 Ragged edges are zeros in LDS: the loads below read nothing past column D of a row, the caller tests the row.
//   k order       mma_step consumes the step's k = 0, 1, then 2, 3, ... 30, 31, each MFMA adding k then k + 1 to every element: with
//                 the steps taken in ascending order an element is ONE fmaf chain over ascending k, whatever the stride.  The
//                 rankings of both baselines rest on that order; it is written here and nowhere else.
//   accumulators  acc[ai][bi][e] of a lane is the product of A row 64 wa + 32 ai + (e & 3) + 8 (e >> 2) + 4 (lane >> 5) (a_row)
//                 and B row 64 wb + 32 bi + (lane & 31) (b_row): a lane holds ONE B row per bi and 16 A rows.
//
// The helpers take pointers and a stride; they own no __shared__ storage and no barrier, so where a kernel stages, aliases and
// synchronises stays readable in the kernel.  Every file pulls this in with `using namespace f32_tile` inside its anonymous namespace.
// The bodies are meant to compile to what the kernels spelled out themselves: compare the device assembly of both files before and after
// a change here.
#pragma once
#include "common.h"

namespace f32_tile {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef f32x16 Acc[2][2];            // [ai][bi]

constexpr int NT = 256;              // threads per workgroup
constexpr int TILE = 128;            // rows of A and of B per workgroup
constexpr int BK = 32;               // k-step
constexpr int LD_QUAD = 129;         // image row stride for transposing element stores
constexpr int LD_ROWS = 160;         // image row stride for 16-byte row stores

struct Wave {
    int lane, wa, wb;
};
__device__ __forceinline__ Wave wave_coords() {
    const int t = threadIdx.x, wave = t >> 6;
    return Wave{t & 63, wave >> 1, wave & 1};
}
__device__ __forceinline__ int a_row(const Wave& w, int ai, int e) { return w.wa * 64 + ai * 32 + (e & 3) + 8 * (e >> 2) + 4 * (w.lane >> 5); }
__device__ __forceinline__ int b_row(const Wave& w, int bi) { return w.wb * 64 + bi * 32 + (w.lane & 31); }

__device__ __forceinline__ void zero(Acc& acc) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
}

// ------------------------------------------------------------------------------------------------ global loads
// row `row` of x, columns [k, k + 4): zero past column D.  `vec`: base 16-byte aligned and ld % 4 == 0.  The caller has checked the
// row, or hands its test in as `row_ok` (zeros for a row that fails it): one predicate with k < D keeps the load behind one branch.
__device__ __forceinline__ float4 load_quad(const float* __restrict__ x, int ld, int row, int k, int D, bool vec, bool row_ok = true) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_ok && k < D) {
        const float* p = x + (size_t)row * ld + k;
        if (vec && k + 4 <= D) {
            v = *reinterpret_cast<const float4*>(p);
        } else {
            v.x = p[0];
            if (k + 1 < D) v.y = p[1];
            if (k + 2 < D) v.z = p[2];
            if (k + 3 < D) v.w = p[3];
        }
    }
    return v;
}
// entries [k, k + 4) of a contiguous fp32 vector of length D, zero past it (element loads: the vector may start anywhere)
__device__ __forceinline__ float4 vec_quad(const float* __restrict__ m, int k, int D) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < D) v.x = m[k];
    if (k + 1 < D) v.y = m[k + 1];
    if (k + 2 < D) v.z = m[k + 2];
    if (k + 3 < D) v.w = m[k + 3];
    return v;
}

// One wave over a row of D floats, lane l at columns l, l + 64, ...: f(value) for each of them; true in every lane when the row
// holds a NaN or an infinity.
template <typename F>
__device__ __forceinline__ bool row_nonfinite(const float* __restrict__ p, int D, int lane, F f) {
    bool bad = false;
    for (int c = lane; c < D; c += 64) {
        const float v = p[c];
        bad |= nonfinite(v);
        f(v);
    }
    return __ballot(bad) != 0ull;
}

// ------------------------------------------------------------------------------------------------ the LDS image
// columns [k, k + 4) of row `row`, as load_quad returned them, into the k-major image S
template <int LD>
__device__ __forceinline__ void store_quad_t(float* S, int k, int row, float4 v) {
    S[(k + 0) * LD + row] = v.x; S[(k + 1) * LD + row] = v.y;
    S[(k + 2) * LD + row] = v.z; S[(k + 3) * LD + row] = v.w;
}

// one k-step: acc += A B^T over the 32 k of the images As and Bs (which may be the same image)
template <int LD>
__device__ __forceinline__ void mma_step(const float* As, const float* Bs, Acc& acc, const Wave& w) {
    const float* ap = As + (w.lane >> 5) * LD + w.wa * 64 + (w.lane & 31);
    const float* bp = Bs + (w.lane >> 5) * LD + w.wb * 64 + (w.lane & 31);
#pragma unroll
    for (int ks = 0; ks < BK; ks += 2) {
        const float a0 = ap[ks * LD], a1 = ap[ks * LD + 32];
        const float b0 = bp[ks * LD], b1 = bp[ks * LD + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------ the result
// f(A row, B row, value) for the lane's 64 elements, in register order (ai, bi, e).  knn.hip's stage store walks the same order with
// its own loops: through a callback that mixes LDS loads with its LDS stores the compiler allocated 189 registers for 154.
template <typename F>
__device__ __forceinline__ void acc_walk(const Acc& acc, const Wave& w, F f) {
#pragma unroll
    for (int ai = 0; ai < 2; ++ai)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int e = 0; e < 16; ++e) f(a_row(w, ai, e), b_row(w, bi), acc[ai][bi][e]);
}

}  // namespace f32_tile
