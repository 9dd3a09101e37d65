// Greedy k-center (farthest-point) selection over the rows of an fp32 feature matrix: idx[0] = start, then m - 1 times the eligible,
// not yet chosen row that lies farthest from its nearest centre, equal distances to the lowest row.  Each centre costs one streaming
// pass over x; the index of the next centre never leaves the device.
//
//   pass t        one launch per centre, t = 0 .. m - 1, chained on the caller's stream.  Centre t is `start` (t = 0) or the row held in
//                 keys[t - 1], the word pass t - 1 reduced into.  The centre's row goes to LDS once per workgroup; a wave takes
//                 CS_W consecutive rows, four at a time (8 KB of loads in flight per wave at D = 512), a workgroup CS_R = 4 CS_W.
//   distance      d2 = sum_d (x_d - c_d)^2 in the difference form: a point next to a centre keeps its distance, integer-valued features
//                 give exact results.  Lane l takes columns 4 l + 256 j + {0, 1, 2, 3} in ascending order as ONE fmaf chain
//                 (s = fmaf(x - c, x - c, s)), then the wave's butterfly sum: a fixed order, the same for 16-byte and for element
//                 loads, at most D + 2 roundings on any term.  Compiled without contraction: nothing but the fmaf written here fuses.
//   state         d2min[i] and assign[i] are updated where the new distance is strictly smaller (the earliest centre keeps a tie);
//                 the centre itself gets d2min = 0 and its own position.  flag[i] in scratch: 0 eligible, 1 holds a NaN or an infinity
//                 (found in pass 0; assign = -1, d2min = NaN, never read again), 2 chosen (never read again).
//   arg-max       key = ordered_bits(d2min) << 32 | (0xFFFFFFFF - row) of every row still eligible after the update: the largest key
//                 is the farthest row, the lowest row among equals.  A wave keeps its largest key in a register (every lane holds the
//                 row's sum, so the key is the same in all of them), the workgroup's four
//                 meet in LDS, one integer atomicMax per workgroup goes to keys[t] -- none where an agent-scope load shows the word
//                 at or above the key already (the word only grows, so an old value skips nothing that could win).  Integer max is
//                 independent of the order of arrival: two runs give the same bytes.  keys[t] == 0 means no eligible row is left:
//                 the passes behind it return at once and write idx = -1, radius = NaN.
//   outputs       workgroup 0 of pass t writes idx[t] and radius[t] from keys[t - 1]; pass 0 counts the non-finite rows with one
//                 integer atomicAdd per workgroup that has any.
// keys and counts are cleared by the call itself (hipMemsetAsync on the stream), flag is written whole by pass 0: a dirty scratch
// changes nothing.  No float atomics, no cooperative launch, no wait between workgroups: every launch is bounded by its own rows.
#include "f32_tile.h"

// the difference and the fmaf chain below are the statement of the distance: no other pair of operations may fuse
#pragma clang fp contract(off)

namespace {

constexpr int CS_NT = 256;                     // threads per workgroup
constexpr int CS_W = 8;                        // rows per wave
constexpr int CS_R = CS_W * (CS_NT / 64);      // rows per workgroup
constexpr int CS_G = 4;                        // rows a wave has in flight
constexpr int CS_D_MAX = 2048;
constexpr int CS_N_MAX = 1 << 24;
constexpr unsigned CS_NAN = 0x7FC00000u, CS_INF = 0x7F800000u;

struct CoresetScratch {                        // byte offsets into the caller's scratch
    size_t keys, flag, total;
};
CoresetScratch coreset_layout(int n, int m) {
    CoresetScratch s;
    s.keys = 0;
    s.flag = s.keys + align_up((size_t)m * 8, 16);
    s.total = s.flag + align_up((size_t)n * 4, 16);
    return s;
}

// columns [k, k + 4) of a row at p (k < D), zeros past column D and for a row that is not `ok`.  VEC: p is 16-byte aligned and D % 4 == 0, so
// the quad is whole.  The two forms are two kernels: in one function the compiler shares the first element's load between them and
// what is left of the 16-byte load is a 4-byte and a 12-byte one.
template <bool VEC>
__device__ __forceinline__ float4 cs_quad(const float* __restrict__ p, int k, int D, bool ok) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
        if (VEC) {
            v = *reinterpret_cast<const float4*>(p + k);
        } else {
            v.x = p[k];
            if (k + 1 < D) v.y = p[k + 1];
            if (k + 2 < D) v.z = p[k + 2];
            if (k + 3 < D) v.w = p[k + 3];
        }
    }
    return v;
}

template <bool FIRST, bool VEC>
__global__ __launch_bounds__(CS_NT) void coreset_pass_kernel(const float* __restrict__ x, int ldx, int n, int D, int t, int start,
                                                             unsigned long long* __restrict__ keys, int* __restrict__ flag,
                                                             int* __restrict__ idx, float* __restrict__ radius, int* __restrict__ assign,
                                                             float* __restrict__ d2min, int* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float cs[CS_D_MAX];
    __shared__ unsigned long long wbest[CS_NT / 64];
    __shared__ int wbad[CS_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int c = start;
    if (!FIRST) {
        const unsigned long long prev = keys[t - 1];                          // complete: the pass that wrote it has ended
        c = prev ? (int)(0xFFFFFFFFu - (unsigned)(prev & 0xFFFFFFFFull)) : -1;
        if (blockIdx.x == 0 && tid == 0) {
            idx[t] = c;
            radius[t] = prev ? from_ordered_bits((unsigned)(prev >> 32)) : __uint_as_float(CS_NAN);
        }
        if (c < 0) return;                                                    // no eligible row is left; uniform over the grid
    } else if (blockIdx.x == 0 && tid == 0) {
        idx[0] = start;
        radius[0] = __uint_as_float(CS_INF);
    }

    const int Dq = (D + 3) & ~3;                                              // the centre, zeros up to the next quad
    for (int k = tid; k < Dq; k += CS_NT) cs[k] = k < D ? x[(size_t)c * ldx + k] : 0.f;
    __syncthreads();

    unsigned long long best = 0ull;
    int nbad = 0;
    const int w0 = blockIdx.x * CS_R + wave * CS_W;
    for (int g = 0; g < CS_W; g += CS_G) {
        int row[CS_G];
        bool live[CS_G];
        float s[CS_G];
        bool bad[CS_G];
#pragma unroll
        for (int j = 0; j < CS_G; ++j) {
            row[j] = w0 + g + j;
            live[j] = row[j] < n;
            if (!FIRST && live[j]) live[j] = __builtin_amdgcn_readfirstlane(flag[row[j]]) == 0;
            s[j] = 0.f;
            bad[j] = false;
        }
        for (int k = lane * 4; k < D; k += 256) {
            const float4 cv = *reinterpret_cast<const float4*>(cs + k);
            float4 v[CS_G];
#pragma unroll
            for (int j = 0; j < CS_G; ++j) v[j] = cs_quad<VEC>(x + (size_t)row[j] * ldx, k, D, live[j]);
#pragma unroll
            for (int j = 0; j < CS_G; ++j) {
                if (FIRST) bad[j] |= nonfinite(v[j].x) | nonfinite(v[j].y) | nonfinite(v[j].z) | nonfinite(v[j].w);
                const float dx = v[j].x - cv.x, dy = v[j].y - cv.y, dz = v[j].z - cv.z, dw = v[j].w - cv.w;
                s[j] = fmaf(dx, dx, s[j]);
                s[j] = fmaf(dy, dy, s[j]);
                s[j] = fmaf(dz, dz, s[j]);
                s[j] = fmaf(dw, dw, s[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < CS_G; ++j) {
            if (!live[j]) continue;                                           // uniform over the wave
            const int i = row[j];
            const float d = wave_sum(s[j]);                                   // the same bits in every lane
            float cur;
            if (FIRST) {
                if (__ballot(bad[j]) != 0ull) {
                    if (lane == 0) {
                        flag[i] = 1;
                        assign[i] = -1;
                        d2min[i] = __uint_as_float(CS_NAN);
                        if (i == c) counts[1] = 1;
                    }
                    ++nbad;
                    continue;
                }
                if (lane == 0) {
                    flag[i] = i == c ? 2 : 0;
                    assign[i] = 0;
                    d2min[i] = d;
                }
                if (i == c) continue;
                cur = d;
            } else {
                if (i == c) {
                    if (lane == 0) {
                        flag[i] = 2;
                        assign[i] = t;
                        d2min[i] = 0.f;
                    }
                    continue;
                }
                cur = d2min[i];
                if (d < cur) {
                    cur = d;
                    if (lane == 0) {
                        assign[i] = t;
                        d2min[i] = d;
                    }
                }
            }
            const unsigned long long key = ((unsigned long long)ordered_bits(cur) << 32) | (0xFFFFFFFFu - (unsigned)i);
            best = key > best ? key : best;
        }
    }
    if (lane == 0) {
        wbest[wave] = best;
        wbad[wave] = nbad;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < CS_NT / 64; ++w) {
            best = wbest[w] > best ? wbest[w] : best;
            nbad += wbad[w];
        }
        if (FIRST && nbad) atomicAdd(&counts[0], nbad);
        if (best && __hip_atomic_load(&keys[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < best) atomicMax(&keys[t], best);
    }
}

bool coreset_in_range(int n, int D, int m) { return n >= 1 && n < CS_N_MAX && D >= 1 && D <= CS_D_MAX && m >= 1 && m <= n; }

}  // namespace

extern "C" size_t eoe_feature_coreset_scratch_bytes(int n, int D, int m) {
    return coreset_in_range(n, D, m) ? coreset_layout(n, m).total : 0;
}

extern "C" int eoe_feature_coreset(const float* x, int ldx, int n, int D, int m, int start, int* idx, float* radius, int* assign, float* d2min,
                                   int* counts, void* scratch, void* stream) {
    EOE_CHECK_ARG(x && idx && radius && assign && d2min && counts && scratch,
                  "feature_coreset: null x, idx, radius, assign, d2min, counts or scratch");
    EOE_CHECK_ARG(D >= 1 && D <= CS_D_MAX, "feature_coreset: D must be in [1, %d], not %d", CS_D_MAX, D);
    EOE_CHECK_ARG(ldx >= D, "feature_coreset: ldx must be at least D = %d, not %d", D, ldx);
    EOE_CHECK_ARG(n >= 1 && n < CS_N_MAX, "feature_coreset: n must be in [1, 2^24), not %d", n);
    EOE_CHECK_ARG(m >= 1 && m <= n, "feature_coreset: m must be in [1, n = %d], not %d", n, m);
    EOE_CHECK_ARG(start >= 0 && start < n, "feature_coreset: start must be in [0, n = %d), not %d", n, start);
    EOE_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)idx & 3) == 0 && ((uintptr_t)radius & 3) == 0 && ((uintptr_t)assign & 3) == 0 &&
                      ((uintptr_t)d2min & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)scratch & 15) == 0,
                  "feature_coreset: x, idx, radius, assign, d2min and counts must be 4-byte aligned, scratch 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const CoresetScratch lay = coreset_layout(n, m);
    char* base = static_cast<char*>(scratch);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + lay.keys);
    int* flag = reinterpret_cast<int*>(base + lay.flag);
    ProfScope ps("feature_coreset", 3.0 * n * (double)D * m, 4.0 * n * (double)D * m, stream);
    hipError_t e = hipMemsetAsync(keys, 0, (size_t)m * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 2 * sizeof(int), st);
    if (e != hipSuccess) return eoe_set_error(EOE_ERR_LAUNCH, "feature_coreset (clear): %s", hipGetErrorString(e));
    const bool vec = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0 && (D & 3) == 0;
    const dim3 grid((unsigned)cdiv(n, CS_R)), block(CS_NT);
    const auto first = vec ? coreset_pass_kernel<true, true> : coreset_pass_kernel<true, false>;
    const auto next = vec ? coreset_pass_kernel<false, true> : coreset_pass_kernel<false, false>;
    hipLaunchKernelGGL(first, grid, block, 0, st, x, ldx, n, D, 0, start, keys, flag, idx, radius, assign, d2min, counts);
    EOE_CHECK_LAUNCH("feature_coreset (pass 0)");
    for (int t = 1; t < m; ++t) {
        hipLaunchKernelGGL(next, grid, block, 0, st, x, ldx, n, D, t, start, keys, flag, idx, radius, assign, d2min, counts);
        EOE_CHECK_LAUNCH("feature_coreset (pass)");
    }
    return 0;
}
