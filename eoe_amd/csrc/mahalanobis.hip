// The Gaussian baseline in feature space: the moments of a set of fp32 feature vectors (mean, scatter matrix, the fourth moment that
// Ledoit-Wolf shrinkage needs) and the squared Mahalanobis distance of query rows, d2 = |W (x - mean)|^2.  Both matrix products run on
// v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate, bit for bit a k-ordered fmaf chain) through the 128 x 128 x 32 tile layer of
// f32_tile.h, which knn.hip uses too: its workgroup shape, k-major operand images, k order and accumulator map.
//
// eoe_feature_moments, six launches:
//   flags         one wave per row: does it hold a NaN or an infinity.  Such a row is excluded from everything below.
//   column sums   a thread per column walks one slice of rows (MH_CS_ROWS or more, at most MH_CS_MAX slices) in ascending order and
//                 adds the used rows in float64: psum[slice][D], and the slice's count of used rows.
//   mean          a thread per column adds the slices in ascending order in float64, divides by the rows used and rounds once to
//                 fp32; counts = {used, excluded}.  No row used: the mean is 0.
//   row norms     one wave per row: |z|^2 of z = x - mean as an fp32 fmaf chain per lane (columns lane, lane + 64, ...) and the wave's
//                 butterfly sum; 0 for an excluded row.
//   scatter       S = Z^T Z.  The reduction runs over the ROWS of x, so a k-major operand tile [32 rows][128 columns] is x as it lies
//                 in memory: 16-byte loads go to LDS as 16-byte stores, z = x - mean formed on the way (no centred copy of x exists;
//                 an excluded row, a row past the slice and a column past D are zeros): the image of row stride 160.  Only the
//                 128 x 128 tiles on or above the diagonal are computed, nt (nt + 1) / 2 of them with nt = ceil(D / 128); a diagonal tile stages one operand and reads
//                 it twice.  The rows are cut into `splits` slices, a pure function of (n, D): the count that brings tiles x splits
//                 to 256 workgroups or just above, one per CU (26 at D = 512, 2 at D = 2048), never more than ceil(n / 32).  Each
//                 (tile, split) workgroup writes its whole fp32 tile to scratch: 17 MB at D = 512, 18 MB at D = 2048, any n
//                 (the scratch size asks for its bound, 255 + tiles of them: 26 MB at most).
//   finish        a workgroup per 32 x 32 block of an upper tile adds the splits in ascending order in float64 and writes the block
//                 and, through LDS, its mirror image (a diagonal tile holds both triangles itself: the fmaf chains of S_ab and S_ba
//                 multiply the same pairs in the same order, so they are equal bit for bit).  One more workgroup adds the squares of
//                 the row norms in float64 in a fixed order: m4.
//
// eoe_mahalanobis_score, three launches:
//   flags         as above, for the query rows.
//   tiles         y = W (x - mean) for 128 queries x 128 rows of W per workgroup: A = W, B = the centred queries (formed while the tile
//                 is staged), the images of row stride 129.  A lane of the result holds ONE query and 16 rows of W: it squares
//                 and adds them in register order (an fmaf chain), adds the other half wave's sum and the other wave's through LDS,
//                 and writes one fp32 partial per (query, column tile) to scratch.  y is never stored.
//                 Partials rather than one workgroup per query tile: at nq = 10 000, D = P = 512 that is 79 x 4 = 316 workgroups on
//                 256 CUs (two or three fit a CU's LDS) against 79.
//                 lower != 0 (P == D, W[j,k] == 0 for k > j): a column tile stops at k = its last row; the skipped steps would add
//                 0 * z to every sum, which changes no y^2 while every fp32 x - mean is finite.
//   sum           a thread per query adds its partials in ascending order; NaN for a flagged query; workgroup 0 counts the flags.
//
// No atomics, fixed orders, every scratch word that is read is written first: two runs give the same bytes under any scratch content.
#include "f32_tile.h"

namespace {

using namespace f32_tile;

constexpr int MH_NT = NT;
constexpr int MH_TILE = TILE;                  // columns of x (moments) / queries and rows of W (score) per workgroup
constexpr int MH_BK = BK;                      // k-step
constexpr int MH_LDM = LD_ROWS;                // moments: x lies k-major in memory, 16-byte row stores
constexpr int MH_LDS = LD_QUAD;                // score: a 16-byte load holds four k of one row, transposing stores
constexpr int MH_D_MAX = 2048;
constexpr int MH_N_MAX = 1 << 30;
constexpr int MH_CS_ROWS = 256;                // rows per slice of the column sums ...
constexpr int MH_CS_MAX = 512;                 // ... unless that makes more slices than this
constexpr int MH_CUS = 256;
constexpr int MH_SUB = 32;                     // the finish kernel's block edge

int mh_tiles_1d(int D) { return cdiv(D, MH_TILE); }
int mh_upper_tiles(int D) { const int nt = mh_tiles_1d(D); return nt * (nt + 1) / 2; }
// rows per scatter slice (a multiple of the k-step) and the number of slices: a pure function of (n, D)
void mh_splits(int n, int D, int* rows_per, int* splits) {
    const int T = mh_upper_tiles(D);
    int s = cdiv(MH_CUS, T);
    const int most = n > 0 ? (int)(((long long)n + MH_BK - 1) / MH_BK) : 1;
    if (s > most) s = most;
    if (s < 1) s = 1;
    long long rp = ((long long)n + s - 1) / s;
    rp = (rp + MH_BK - 1) / MH_BK * MH_BK;
    if (rp < MH_BK) rp = MH_BK;
    *rows_per = (int)rp;
    *splits = n > 0 ? (int)(((long long)n + rp - 1) / rp) : 1;
}
void mh_cs_slices(int n, int* rows_per, int* slices) {
    long long rp = MH_CS_ROWS;
    if (((long long)n + rp - 1) / rp > MH_CS_MAX) rp = ((long long)n + MH_CS_MAX - 1) / MH_CS_MAX;
    *rows_per = (int)rp;
    *slices = n > 0 ? (int)(((long long)n + rp - 1) / rp) : 1;
}

struct MomScratch {                            // byte offsets into the caller's scratch
    size_t flag, rq, pcnt, psum, part, total;
};
// The regions are sized by bounds that grow with n and with D, which the counts themselves do not (a longer slice can mean fewer of
// them): slices <= min(ceil(n / 256), 512), tiles x splits <= min(tiles x ceil(n / 32), 255 + tiles).
MomScratch mom_layout(int n, int D) {
    const long long T = mh_upper_tiles(D);
    long long slices = ((long long)n + MH_CS_ROWS - 1) / MH_CS_ROWS;
    slices = slices < 1 ? 1 : (slices > MH_CS_MAX ? MH_CS_MAX : slices);
    long long ksteps = ((long long)n + MH_BK - 1) / MH_BK;
    if (ksteps < 1) ksteps = 1;
    const long long parts = T * ksteps < MH_CUS - 1 + T ? T * ksteps : MH_CUS - 1 + T;
    MomScratch s;
    s.flag = 0;
    s.rq = s.flag + align_up((size_t)n * 4, 16);
    s.pcnt = s.rq + align_up((size_t)n * 4, 16);
    s.psum = s.pcnt + align_up((size_t)slices * 4, 16);
    s.part = s.psum + align_up((size_t)slices * D * 8, 16);
    s.total = s.part + (size_t)parts * MH_TILE * MH_TILE * 4 + 16;
    return s;
}
struct ScoreScratch {
    size_t flag, part, total;
};
ScoreScratch score_layout(int nq, int P) {
    ScoreScratch s;
    s.flag = 0;
    s.part = s.flag + align_up((size_t)nq * 4, 16);
    s.total = s.part + align_up((size_t)nq * cdiv(P, MH_TILE) * 4, 16) + 16;
    return s;
}

// one wave per row: 1 for a row that holds a NaN or an infinity
__global__ __launch_bounds__(MH_NT) void mh_flag_kernel(const float* __restrict__ x, int ld, int n, int D, int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (MH_NT / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const bool any = row_nonfinite(x + (size_t)row * ld, D, lane, [](float) {});
    if (lane == 0) flag[row] = any ? 1 : 0;
}

// blockIdx.x: 256 columns, blockIdx.y: a slice of rows.  psum[slice][D] in float64, pcnt[slice] = used rows of the slice.
__global__ __launch_bounds__(MH_NT) void mh_colsum_kernel(const float* __restrict__ x, int ld, int n, int D, int rows_per,
                                                          const int* __restrict__ flag, double* __restrict__ psum, int* __restrict__ pcnt) {
    const int c = blockIdx.x * MH_NT + threadIdx.x, sl = blockIdx.y;
    const long long r0 = (long long)sl * rows_per;
    const long long r1 = r0 + rows_per < n ? r0 + rows_per : n;
    double acc = 0.0;
    int used = 0;
    for (long long r = r0; r < r1; ++r) {
        if (flag[r]) continue;                                                // uniform over the workgroup
        ++used;
        if (c < D) acc += (double)x[(size_t)r * ld + c];
    }
    if (c < D) psum[(size_t)sl * D + c] = acc;
    if (c == 0) pcnt[sl] = used;
}

__global__ __launch_bounds__(MH_NT) void mh_mean_kernel(int n, int D, int slices, const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                        float* __restrict__ mean, int* __restrict__ counts) {
    const int c = blockIdx.x * MH_NT + threadIdx.x;
    long long used = 0;
    for (int s = 0; s < slices; ++s) used += pcnt[s];
    if (c == 0) { counts[0] = (int)used; counts[1] = (int)(n - used); }
    if (c >= D) return;
    double acc = 0.0;
    for (int s = 0; s < slices; ++s) acc += psum[(size_t)s * D + c];
    mean[c] = used > 0 ? (float)(acc / (double)used) : 0.f;
}

// one wave per row: |x - mean|^2 in fp32, 0 for an excluded row
__global__ __launch_bounds__(MH_NT) void mh_rownorm_kernel(const float* __restrict__ x, int ld, int n, int D, const float* __restrict__ mean,
                                                           const int* __restrict__ flag, float* __restrict__ rq) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (MH_NT / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    float s = 0.f;
    if (!flag[row]) {                                                         // uniform over the wave
        const float* p = x + (size_t)row * ld;
        for (int c = lane; c < D; c += 64) {
            const float z = p[c] - mean[c];
            s = fmaf(z, z, s);
        }
        s = wave_sum(s);
    }
    if (lane == 0) rq[row] = s;
}

// (ta, tb), ta <= tb, of upper tile `t` in row-major order over nt x nt tiles
__device__ __forceinline__ void mh_tile_pair(int t, int nt, int& ta, int& tb) {
    ta = 0;
    while (t >= nt - ta) { t -= nt - ta; ++ta; }
    tb = ta + t;
}

__global__ __launch_bounds__(MH_NT) void mh_scatter_kernel(const float* __restrict__ x, int ld, int n, int D, int nt, int splits, int rows_per,
                                                           int vec, const float* __restrict__ mean, const int* __restrict__ flag,
                                                           float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[MH_BK * MH_LDM];
    __shared__ __attribute__((aligned(16))) float Bs[MH_BK * MH_LDM];
    const int t = threadIdx.x;
    const Wave w = wave_coords();
    const int tile = (int)(blockIdx.x / (unsigned)splits), sp = (int)(blockIdx.x % (unsigned)splits);
    int ta, tb;
    mh_tile_pair(tile, nt, ta, tb);
    const bool diag = ta == tb;
    const int ca = ta * MH_TILE + (t & 31) * 4, cb = tb * MH_TILE + (t & 31) * 4;   // this thread's column quad of either operand
    const int lrow = t >> 5;                                                        // its first row of a k-step (then + 8)
    const float4 ma = vec_quad(mean, ca, D), mb = vec_quad(mean, cb, D);
    const long long row0 = (long long)sp * rows_per;
    const long long row1 = row0 + rows_per < n ? row0 + rows_per : n;
    const int nkt = row1 > row0 ? (int)((row1 - row0 + MH_BK - 1) / MH_BK) : 0;

    Acc acc;
    zero(acc);
    float4 ra[4], rb[4];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long r = row0 + (long long)kt * MH_BK + lrow + 8 * j;
            ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            rb[j] = ra[j];
            if (r < row1 && !flag[r]) {                                       // past column D both x and the mean read as 0
                const float4 v = load_quad(x, ld, (int)r, ca, D, vec != 0);
                ra[j] = make_float4(v.x - ma.x, v.y - ma.y, v.z - ma.z, v.w - ma.w);
                if (!diag) {
                    const float4 u = load_quad(x, ld, (int)r, cb, D, vec != 0);
                    rb[j] = make_float4(u.x - mb.x, u.y - mb.y, u.z - mb.z, u.w - mb.w);
                }
            }
        }
    };
    if (nkt > 0) fetch(0);
    const float* bsrc = diag ? As : Bs;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();                                                      // the last reads of the operand tiles are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int off = (lrow + 8 * j) * MH_LDM + (t & 31) * 4;
            *reinterpret_cast<float4*>(As + off) = ra[j];
            if (!diag) *reinterpret_cast<float4*>(Bs + off) = rb[j];
        }
        __syncthreads();
        if (kt + 1 < nkt) fetch(kt + 1);
        mma_step<MH_LDM>(As, bsrc, acc, w);
    }
    float* out = part + (size_t)blockIdx.x * (MH_TILE * MH_TILE);            // [tile][split][128 a][128 b], the whole tile
    acc_walk(acc, w, [&](int al, int bl, float v) { out[al * MH_TILE + bl] = v; });
}

// blocks [0, tiles * 16): a 32 x 32 block of an upper tile; the last block: m4
__global__ __launch_bounds__(MH_NT) void mh_finish_kernel(int n, int D, int nt, int tiles, int splits, const float* __restrict__ part,
                                                          const float* __restrict__ rq, double* __restrict__ S, double* __restrict__ m4) {
    __shared__ double buf[MH_SUB][MH_SUB + 1];
    __shared__ double red[MH_NT];
    const int t = threadIdx.x;
    constexpr int PER = MH_TILE / MH_SUB;                                     // 4 x 4 blocks per tile
    if ((int)blockIdx.x == tiles * PER * PER) {
        double acc = 0.0;
        for (long long i = t; i < n; i += MH_NT) {
            const double q = (double)rq[i];
            acc += q * q;
        }
        acc = block_tree_sum<MH_NT>(acc, red);
        if (t == 0) m4[0] = acc;
        return;
    }
    const int tile = blockIdx.x / (PER * PER), sub = blockIdx.x % (PER * PER);
    int ta, tb;
    mh_tile_pair(tile, nt, ta, tb);
    const int a0 = (sub / PER) * MH_SUB, b0 = (sub % PER) * MH_SUB;           // within the tile
    const int ga = ta * MH_TILE + a0, gb = tb * MH_TILE + b0;
    if (ga >= D || gb >= D) return;                                           // uniform over the workgroup
    const int c = t & 31, r = t >> 5;
    const float* base = part + (size_t)tile * splits * (MH_TILE * MH_TILE);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rr = r + 8 * j;
        const float* p = base + (a0 + rr) * MH_TILE + b0 + c;
        double acc = 0.0;
        for (int s = 0; s < splits; ++s) acc += (double)p[(size_t)s * (MH_TILE * MH_TILE)];
        buf[rr][c] = acc;
        if (ga + rr < D && gb + c < D) S[(size_t)(ga + rr) * D + gb + c] = acc;
    }
    if (ta == tb) return;                                                     // a diagonal tile holds both of its triangles
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rr = r + 8 * j;                                             // the mirror image: row gb + rr, column ga + c
        if (gb + rr < D && ga + c < D) S[(size_t)(gb + rr) * D + ga + c] = buf[c][rr];
    }
}

__global__ __launch_bounds__(MH_NT) void mh_score_kernel(const float* __restrict__ x, int ldx, int nq, int D, const float* __restrict__ mean,
                                                         const float* __restrict__ W, int ldw, int P, int ptiles, int lower, int vecx, int vecw,
                                                         float* __restrict__ part) {
    __shared__ float As[MH_BK * MH_LDS];                                      // [k][row of W]
    __shared__ float Bs[MH_BK * MH_LDS];                                      // [k][query]
    __shared__ float red[MH_TILE];
    const int t = threadIdx.x;
    const Wave w = wave_coords();                                             // the wave's 64 rows of W (A) x 64 queries (B)
    const int pt = (int)(blockIdx.x % (unsigned)ptiles), qb = (int)(blockIdx.x / (unsigned)ptiles);
    const int q0 = qb * MH_TILE, p0 = pt * MH_TILE;
    const int lk = (t & 7) * 4, lrow = t >> 3;                                // loads: k quad and first row (then + 32)
    int kend = D;
    if (lower && p0 + MH_TILE < D) kend = p0 + MH_TILE;                       // W[j, k] == 0 for k > j: nothing past the tile's last row
    const int nkt = (kend + MH_BK - 1) / MH_BK;

    Acc acc;
    zero(acc);
    float4 ra[4], rb[4];
    auto fetch = [&](int kt) {
        const int kk = kt * MH_BK + lk;
        const float4 m = vec_quad(mean, kk, D);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int wrow = p0 + lrow + 32 * j, qrow = q0 + lrow + 32 * j;
            ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            rb[j] = ra[j];
            if (wrow < P) ra[j] = load_quad(W, ldw, wrow, kk, D, vecw != 0);
            if (qrow < nq) {
                const float4 v = load_quad(x, ldx, qrow, kk, D, vecx != 0);
                rb[j] = make_float4(v.x - m.x, v.y - m.y, v.z - m.z, v.w - m.w);       // past column D both are 0
            }
        }
    };
    fetch(0);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            store_quad_t<MH_LDS>(As, lk, lrow + 32 * j, ra[j]);
            store_quad_t<MH_LDS>(Bs, lk, lrow + 32 * j, rb[j]);
        }
        __syncthreads();
        if (kt + 1 < nkt) fetch(kt + 1);
        mma_step<MH_LDS>(As, Bs, acc, w);
    }
    // a lane holds query b_row(w, qi) and 2 x 16 rows of W: square and add in register order (qi outer; ri, e inner: part of the
    // result, so no acc_walk here), then the other half wave, then the other wave
    const int lane = w.lane, wr = w.wa;
    float s[2];
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
        float v = 0.f;
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int e = 0; e < 16; ++e) v = fmaf(acc[ri][qi][e], acc[ri][qi][e], v);
        s[qi] = v + __shfl_xor(v, 32, 64);
    }
    if (wr == 1 && lane < 32) {
        red[b_row(w, 0)] = s[0];
        red[b_row(w, 1)] = s[1];
    }
    __syncthreads();
    if (wr == 0 && lane < 32) {
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            const int ql = b_row(w, qi);
            if (q0 + ql < nq) part[(size_t)(q0 + ql) * ptiles + pt] = s[qi] + red[ql];
        }
    }
}

__global__ __launch_bounds__(MH_NT) void mh_score_sum_kernel(int nq, int ptiles, const float* __restrict__ part, const int* __restrict__ flag,
                                                             float* __restrict__ d2, int* __restrict__ count) {
    __shared__ int red[MH_NT];
    const int t = threadIdx.x;
    const long long q = (long long)blockIdx.x * MH_NT + t;
    if (q < nq) {
        float acc = 0.f;
        const float* p = part + (size_t)q * ptiles;
        for (int i = 0; i < ptiles; ++i) acc += p[i];
        d2[q] = flag[q] ? __uint_as_float(0x7FC00000u) : acc;
    }
    if (blockIdx.x == 0) {
        int c = 0;
        for (long long i = t; i < nq; i += MH_NT) c += flag[i];
        c = block_tree_sum<MH_NT>(c, red);
        if (t == 0) count[0] = c;
    }
}

bool mom_in_range(int n, int D) { return n >= 0 && n <= MH_N_MAX && D >= 1 && D <= MH_D_MAX; }
bool score_in_range(int nq, int D, int P) { return nq >= 0 && nq <= MH_N_MAX && D >= 1 && D <= MH_D_MAX && P >= 1 && P <= MH_D_MAX; }

}  // namespace

extern "C" size_t eoe_feature_moments_scratch_bytes(int n, int D) { return mom_in_range(n, D) ? mom_layout(n, D).total : 0; }

extern "C" int eoe_feature_moments(const float* x, int ld, int n, int D, float* mean, double* scatter, double* m4, int* counts, void* scratch,
                                   void* stream) {
    EOE_CHECK_ARG(x && mean && scatter && m4 && counts && scratch, "feature_moments: null x, mean, scatter, m4, counts or scratch");
    EOE_CHECK_ARG(D >= 1 && D <= MH_D_MAX, "feature_moments: D must be in [1, %d], not %d", MH_D_MAX, D);
    EOE_CHECK_ARG(ld >= D, "feature_moments: ld must be at least D = %d, not %d", D, ld);
    EOE_CHECK_ARG(n >= 0 && n <= MH_N_MAX, "feature_moments: n must be in [0, 2^30], not %d", n);
    EOE_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)mean & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)scatter & 7) == 0 &&
                      ((uintptr_t)m4 & 7) == 0 && ((uintptr_t)scratch & 15) == 0,
                  "feature_moments: x, mean and counts must be 4-byte aligned, scatter and m4 8-byte aligned, scratch 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const MomScratch lay = mom_layout(n, D);
    char* base = static_cast<char*>(scratch);
    int* flag = reinterpret_cast<int*>(base + lay.flag);
    float* rq = reinterpret_cast<float*>(base + lay.rq);
    int* pcnt = reinterpret_cast<int*>(base + lay.pcnt);
    double* psum = reinterpret_cast<double*>(base + lay.psum);
    float* part = reinterpret_cast<float*>(base + lay.part);
    int rp, splits, crp, slices;
    mh_splits(n, D, &rp, &splits);
    mh_cs_slices(n, &crp, &slices);
    const int nt = mh_tiles_1d(D), tiles = mh_upper_tiles(D);
    const unsigned row_blocks = (unsigned)(((long long)n + MH_NT / 64 - 1) / (MH_NT / 64));
    ProfScope ps("feature_moments", (double)n * D * (D + 1), 4.0 * 4.0 * (double)n * D, stream);
    if (n > 0) {
        hipLaunchKernelGGL(mh_flag_kernel, dim3(row_blocks), dim3(MH_NT), 0, st, x, ld, n, D, flag);
        EOE_CHECK_LAUNCH("feature_moments (flags)");
    }
    hipLaunchKernelGGL(mh_colsum_kernel, dim3((unsigned)cdiv(D, MH_NT), (unsigned)slices), dim3(MH_NT), 0, st, x, ld, n, D, crp, (const int*)flag,
                       psum, pcnt);
    EOE_CHECK_LAUNCH("feature_moments (column sums)");
    hipLaunchKernelGGL(mh_mean_kernel, dim3((unsigned)cdiv(D, MH_NT)), dim3(MH_NT), 0, st, n, D, slices, (const double*)psum, (const int*)pcnt, mean,
                       counts);
    EOE_CHECK_LAUNCH("feature_moments (mean)");
    if (n > 0) {
        hipLaunchKernelGGL(mh_rownorm_kernel, dim3(row_blocks), dim3(MH_NT), 0, st, x, ld, n, D, (const float*)mean, (const int*)flag, rq);
        EOE_CHECK_LAUNCH("feature_moments (row norms)");
    }
    const int vec = ((uintptr_t)x & 15) == 0 && (ld & 3) == 0;
    hipLaunchKernelGGL(mh_scatter_kernel, dim3((unsigned)(tiles * splits)), dim3(MH_NT), 0, st, x, ld, n, D, nt, splits, rp, vec, (const float*)mean,
                       (const int*)flag, part);
    EOE_CHECK_LAUNCH("feature_moments (scatter)");
    hipLaunchKernelGGL(mh_finish_kernel, dim3((unsigned)(tiles * 16 + 1)), dim3(MH_NT), 0, st, n, D, nt, tiles, splits, (const float*)part,
                       (const float*)rq, scatter, m4);
    EOE_CHECK_LAUNCH("feature_moments (finish)");
    return 0;
}

extern "C" size_t eoe_mahalanobis_score_scratch_bytes(int nq, int D, int P) {
    return score_in_range(nq, D, P) ? score_layout(nq, P).total : 0;
}

extern "C" int eoe_mahalanobis_score(const float* x, int ldx, int nq, int D, const float* mean, const float* W, int ldw, int P, int lower,
                                     float* d2, int* count, void* scratch, void* stream) {
    EOE_CHECK_ARG(x && mean && W && d2 && count && scratch, "mahalanobis_score: null x, mean, W, d2, count or scratch");
    EOE_CHECK_ARG(D >= 1 && D <= MH_D_MAX, "mahalanobis_score: D must be in [1, %d], not %d", MH_D_MAX, D);
    EOE_CHECK_ARG(P >= 1 && P <= MH_D_MAX, "mahalanobis_score: P must be in [1, %d], not %d", MH_D_MAX, P);
    EOE_CHECK_ARG(ldx >= D, "mahalanobis_score: ldx must be at least D = %d, not %d", D, ldx);
    EOE_CHECK_ARG(ldw >= D, "mahalanobis_score: ldw must be at least D = %d, not %d", D, ldw);
    EOE_CHECK_ARG(!lower || P == D, "mahalanobis_score: lower needs a square W (P == D), not P = %d with D = %d", P, D);
    EOE_CHECK_ARG(nq >= 0 && nq <= MH_N_MAX, "mahalanobis_score: nq must be in [0, 2^30], not %d", nq);
    EOE_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)mean & 3) == 0 && ((uintptr_t)W & 3) == 0 && ((uintptr_t)d2 & 3) == 0 &&
                      ((uintptr_t)count & 3) == 0 && ((uintptr_t)scratch & 15) == 0,
                  "mahalanobis_score: x, mean, W, d2 and count must be 4-byte aligned, scratch 16-byte aligned");
    if (nq == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const ScoreScratch lay = score_layout(nq, P);
    char* base = static_cast<char*>(scratch);
    int* flag = reinterpret_cast<int*>(base + lay.flag);
    float* part = reinterpret_cast<float*>(base + lay.part);
    const int ptiles = cdiv(P, MH_TILE);
    const long long blocks = (long long)cdiv(nq, MH_TILE) * ptiles;
    ProfScope ps("mahalanobis_score", 2.0 * nq * (double)P * D, 4.0 * ((double)nq + P) * D, stream);
    hipLaunchKernelGGL(mh_flag_kernel, dim3((unsigned)(((long long)nq + MH_NT / 64 - 1) / (MH_NT / 64))), dim3(MH_NT), 0, st, x, ldx, nq, D, flag);
    EOE_CHECK_LAUNCH("mahalanobis_score (flags)");
    const int vecx = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0, vecw = ((uintptr_t)W & 15) == 0 && (ldw & 3) == 0;
    hipLaunchKernelGGL(mh_score_kernel, dim3((unsigned)blocks), dim3(MH_NT), 0, st, x, ldx, nq, D, mean, W, ldw, P, ptiles, lower ? 1 : 0, vecx, vecw,
                       part);
    EOE_CHECK_LAUNCH("mahalanobis_score (tiles)");
    hipLaunchKernelGGL(mh_score_sum_kernel, dim3((unsigned)cdiv(nq, MH_NT)), dim3(MH_NT), 0, st, nq, ptiles, (const float*)part, (const int*)flag, d2,
                       count);
    EOE_CHECK_LAUNCH("mahalanobis_score (sum)");
    return 0;
}
