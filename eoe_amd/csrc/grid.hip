// Image grids composed on the device: the picture the reference's `Logger.logimg` (`utils/logger.py:202-295`) hands to `cv2.imwrite`,
// without pulling the images through the host.  The reference stacks float tensors on the host, resizes them with `F.interpolate`,
// normalises each image (`make_grid(normalize=True, scale_each=True)`, or its own min / max rule under `mark`), tiles them and
// multiplies by 255; here the images already sit in HBM (the trainer's fp32 batches, the uint8 OE pool, a ragged arena with its
// centre windows), so one launch pair gathers the listed rows where they lie, resizes, normalises, tiles and writes the finished
// uint8 [Hg, Wg, 3] picture, and one copy back follows.
//
// Layout of a picture of `per` cells of ch x cw (the cell is the image, or maxres x maxres when a side exceeds maxres):
//   xmaps = min(nrow, per), ymaps = ceil(per / xmaps), Hg = (ch + pad) * ymaps + pad, Wg = (cw + pad) * xmaps + pad;
//   cell k starts at (pad + (k / xmaps) * (ch + pad), pad + (k % xmaps) * (cw + pad)); padding and unused cells are 0; a 1-channel
//   image fills the three channels; sep_height black rows are inserted in front of row sep_pos (logger.py:276-282), so the picture
//   has Hg + sep_height rows.  `groups` pictures of `per` cells each lie back to back in one buffer (n = groups * per cells).
// The cells are described by a device table int32 [n, 4] = (row, top, left, mark): the row of the source set (a row outside
//   [0, n_src) is an all-zero cell, never a dereference), the window origin of the ragged form relative to the unpadded image (bytes
//   outside the image are 0, as eoe_pool_sqdist_ragged_u8 reads them), and the frame colour 0xRRGGBB or -1.
// Two launches.  grid_minmax_kernel: one workgroup per cell, min / max over the cell's values AFTER the resize, shuffle reduction, no
//   atomics.  grid_compose_kernel: one thread per 4 output bytes, one dword store (the buffer's last 1-3 bytes: byte stores).  Both
//   call cell_value(), and the file is compiled without floating-point contraction, so the value the minimum was taken from is
//   the value that is normalised: the minimum maps to exactly 0 and the maximum to exactly 255.  All arithmetic is fp32 in the
//   reference's order, (x - lo) / d * 255 with an IEEE division.
// Resize: torch's bilinear rule (align_corners=False, no antialias): src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out
//   in fp32, the second tap clamped to the last index, value = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11).
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int GR_NT = 256;
enum { GR_F32 = 0, GR_U8 = 1, GR_RAGGED = 2 };

struct GridSrc {
    const void* base;                 // fp32 NCHW [n_src, C, h, w], uint8 NHWC [n_src, h, w, C], or the ragged arena
    const long long* offsets;         // ragged: where image i starts;  sizes: (H_i, W_i)
    const int* sizes;
    long long arena_bytes, n_src;
    int form, C, h, w;                // h x w: the source image (ragged: the window)
    int ch, cw, resize;               // the cell
    float sy, sx;                     // (float)h / ch, (float)w / cw
};

struct GridLayout {
    int per, xmaps, ymaps, pad, rows_out, Wg, sep_pos, sep_h, marked;
    long long total;                  // bytes of all pictures
};

// source pixel (c, y, x) of the cell described by t = (row, top, left, mark), in the [0, 1] scale of ToTensor for the uint8 forms
__device__ __forceinline__ float src_pixel(const GridSrc& s, const int* __restrict__ t, int c, int y, int x) {
    const int row = t[0];
    if (row < 0 || row >= s.n_src) return 0.0f;
    if (s.form == GR_F32) return static_cast<const float*>(s.base)[(((size_t)row * s.C + c) * s.h + y) * s.w + x];
    const uint8_t* u8 = static_cast<const uint8_t*>(s.base);
    if (s.form == GR_U8) return (float)u8[(((size_t)row * s.h + y) * s.w + x) * s.C + c] / 255.0f;
    const long long off = s.offsets[row];
    const int H = s.sizes[2 * row], W = s.sizes[2 * row + 1];
    const bool held = H > 0 && W > 0 && (long long)W * s.C < (1ll << 30) && off >= 0 && off <= s.arena_bytes &&
                      (long long)H * ((long long)W * s.C) <= s.arena_bytes - off;
    if (!held) return 0.0f;
    // the origin clamped to [-window, extent]: beyond that the window is wholly outside either way, and the sums cannot overflow
    const int r = y + max(-s.h, min(t[1], H)), q = x + max(-s.w, min(t[2], W));
    if (r < 0 || r >= H || q < 0 || q >= W) return 0.0f;
    return (float)u8[(size_t)off + ((size_t)r * W + q) * s.C + c] / 255.0f;
}

// the value of cell pixel (c, y, x): the image itself, or torch's bilinear interpolation of it
__device__ __forceinline__ float cell_value(const GridSrc& s, const int* __restrict__ t, int c, int y, int x) {
    if (!s.resize) return src_pixel(s, t, c, y, x);
    float fy = s.sy * ((float)y + 0.5f) - 0.5f, fx = s.sx * ((float)x + 0.5f) - 0.5f;
    fy = fy < 0.0f ? 0.0f : fy;
    fx = fx < 0.0f ? 0.0f : fx;
    const int y0 = min((int)fy, s.h - 1), x0 = min((int)fx, s.w - 1);
    const int y1 = y0 + (y0 < s.h - 1 ? 1 : 0), x1 = x0 + (x0 < s.w - 1 ? 1 : 0);
    const float ly1 = fminf(fmaxf(fy - (float)y0, 0.0f), 1.0f), lx1 = fminf(fmaxf(fx - (float)x0, 0.0f), 1.0f);
    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    const float p00 = src_pixel(s, t, c, y0, x0), p01 = src_pixel(s, t, c, y0, x1);
    const float p10 = src_pixel(s, t, c, y1, x0), p11 = src_pixel(s, t, c, y1, x1);
    return ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
}

// grid: one workgroup per cell; minmax[2 k] = min, minmax[2 k + 1] = max over the C * ch * cw values of cell k
__global__ __launch_bounds__(GR_NT) void grid_minmax_kernel(GridSrc s, const int* __restrict__ table, float* __restrict__ minmax) {
    __shared__ float red[2 * (GR_NT / 64)];
    const int k = blockIdx.x, t = threadIdx.x, plane = s.ch * s.cw, count = s.C * plane;
    const int* tk = table + 4 * (size_t)k;
    float lo = INFINITY, hi = -INFINITY;
    for (int e = t; e < count; e += GR_NT) {
        const int c = e / plane, p = e - c * plane, y = p / s.cw;
        const float v = cell_value(s, tk, c, y, p - y * s.cw);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((t & 63) == 0) red[2 * (t >> 6)] = lo, red[2 * (t >> 6) + 1] = hi;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < GR_NT / 64; ++w) lo = fminf(lo, red[2 * w]), hi = fmaxf(hi, red[2 * w + 1]);
        minmax[2 * (size_t)k] = lo;
        minmax[2 * (size_t)k + 1] = hi;
    }
}

// byte `flat` of the pictures
__device__ __forceinline__ unsigned grid_byte(const GridSrc& s, const GridLayout& L, const int* __restrict__ table,
                                              const float* __restrict__ minmax, long long flat) {
    const int rowb = L.Wg * 3;
    const long long pic = (long long)L.rows_out * rowb;
    const int g = (int)(flat / pic), r = (int)(flat - g * pic);
    int Y = r / rowb;
    const int rem = r - Y * rowb, X = rem / 3, c3 = rem - X * 3;
    if (L.sep_h > 0 && Y >= L.sep_pos) {
        if (Y < L.sep_pos + L.sep_h) return 0u;
        Y -= L.sep_h;
    }
    const int cr = Y / (s.ch + L.pad), yy = Y - cr * (s.ch + L.pad) - L.pad;
    const int cc = X / (s.cw + L.pad), xx = X - cc * (s.cw + L.pad) - L.pad;
    if (yy < 0 || xx < 0 || cr >= L.ymaps || cc >= L.xmaps || cr * L.xmaps + cc >= L.per) return 0u;
    const size_t k = (size_t)g * L.per + cr * L.xmaps + cc;
    const int* tk = table + 4 * k;
    if (L.marked && tk[3] >= 0 && (yy == 0 || yy == s.ch - 1 || xx == 0 || xx == s.cw - 1)) return ((unsigned)tk[3] >> (8 * (2 - c3))) & 255u;
    const float lo = minmax[2 * k], hi = minmax[2 * k + 1];
    float x = cell_value(s, tk, s.C == 1 ? 0 : c3, yy, xx), v;
    if (L.marked) {                               // logger.py:238-239, no epsilon; a constant image (0 / 0 there) is all 0
        const float d = hi - lo;
        v = d > 0.0f ? (x - lo) / d : 0.0f;
    } else {                                      // make_grid's norm_range
        x = fminf(fmaxf(x, lo), hi);
        v = (x - lo) / fmaxf(hi - lo, 1e-5f);
    }
    return (unsigned)(int)(v * 255.0f) & 255u;
}

__global__ __launch_bounds__(GR_NT) void grid_compose_kernel(GridSrc s, GridLayout L, const int* __restrict__ table,
                                                             const float* __restrict__ minmax, uint8_t* __restrict__ out) {
    const long long i = ((long long)blockIdx.x * GR_NT + threadIdx.x) * 4;
    if (i >= L.total) return;
    if (i + 4 <= L.total) {
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) word |= grid_byte(s, L, table, minmax, i + b) << (8 * b);
        *reinterpret_cast<unsigned*>(out + i) = word;
    } else {
        for (long long j = i; j < L.total; ++j) out[j] = (uint8_t)grid_byte(s, L, table, minmax, j);
    }
}

// checks the arguments all three forms share, fills the layout and launches; `s` comes with base / form / C / h / w / n_src set
int compose(const char* who, GridSrc s, const int32_t* table, int n, int groups, int nrow, int pad, int maxres, int sep_height,
            int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes, void* stream) {
    EOE_CHECK_ARG(s.C == 1 || s.C == 3, "%s: C must be 1 or 3, not %d", who, s.C);
    EOE_CHECK_ARG(nrow >= 1, "%s: nrow must be at least 1, not %d", who, nrow);
    EOE_CHECK_ARG(pad >= 0 && pad <= 4096, "%s: pad must be in [0, 4096], not %d", who, pad);
    EOE_CHECK_ARG(maxres >= 1 && maxres <= 32768, "%s: maxres must be in [1, 32768], not %d", who, maxres);
    EOE_CHECK_ARG(s.h >= 1 && s.w >= 1 && s.h <= 32768 && s.w <= 32768, "%s: images of %d x %d (h, w in [1, 32768])", who, s.h, s.w);
    EOE_CHECK_ARG(n >= 0 && groups >= 1 && n % groups == 0, "%s: n (%d cells) must be a non-negative multiple of groups (%d)", who, n, groups);
    EOE_CHECK_ARG(sep_height >= 0 && sep_height <= 32768 && sep_at >= 0, "%s: row_sep_at of (%d, %d)", who, sep_height, sep_at);
    EOE_CHECK_ARG(s.n_src >= 0 && s.n_src < (1ll << 31), "%s: n_src must be in [0, 2^31), not %lld", who, s.n_src);
    if (n == 0) {
        EOE_CHECK_ARG(out_bytes == 0, "%s: n = 0 is an empty picture, not %lld bytes", who, (long long)out_bytes);
        return 0;
    }
    EOE_CHECK_ARG(s.base && table && minmax && out, "%s: null source, table, minmax or output", who);
    s.resize = (s.h > maxres || s.w > maxres) ? 1 : 0;
    s.ch = s.resize ? maxres : s.h;
    s.cw = s.resize ? maxres : s.w;
    s.sy = (float)s.h / s.ch;
    s.sx = (float)s.w / s.cw;
    const long long cell = (long long)s.C * s.ch * s.cw;
    EOE_CHECK_ARG((long long)n * cell < (1ll << 31), "%s: n * cell = %d x %lld values exceed 32-bit indexing", who, n, cell);
    GridLayout L;
    L.per = n / groups;
    L.xmaps = nrow < L.per ? nrow : L.per;
    L.ymaps = (L.per + L.xmaps - 1) / L.xmaps;
    L.pad = pad;
    const long long Hg = (long long)(s.ch + pad) * L.ymaps + pad, Wg = (long long)(s.cw + pad) * L.xmaps + pad;
    const long long pos = (long long)(s.ch + pad) * sep_at + pad / 2;
    const long long total = (Hg + sep_height) * Wg * 3 * groups;
    EOE_CHECK_ARG(total < (1ll << 31), "%s: n = %d cells make pictures of %lld bytes, beyond 32-bit indexing", who, n, total);
    EOE_CHECK_ARG(out_bytes == total, "%s: out of %lld bytes, the pictures have %lld", who, (long long)out_bytes, total);
    EOE_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)minmax & 3) == 0 && ((uintptr_t)table & 3) == 0,
                  "%s: out, minmax and table must be 4-byte aligned", who);
    L.rows_out = (int)(Hg + sep_height);
    L.Wg = (int)Wg;
    L.sep_h = sep_height;
    L.sep_pos = (int)(pos < Hg ? pos : Hg);           // t[:pos] of a shorter picture is all of it: the separator goes last
    L.marked = marked ? 1 : 0;
    L.total = total;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(who, 8.0 * (double)n * (double)cell, (double)n * (double)cell * (s.form == GR_F32 ? 4.0 : 1.0) + (double)total, stream);
    hipLaunchKernelGGL(grid_minmax_kernel, dim3((unsigned)n), dim3(GR_NT), 0, st, s, (const int*)table, minmax);
    EOE_CHECK_LAUNCH(who);
    const long long words = (total + 3) / 4;
    hipLaunchKernelGGL(grid_compose_kernel, dim3((unsigned)((words + GR_NT - 1) / GR_NT)), dim3(GR_NT), 0, st, s, L, (const int*)table,
                       (const float*)minmax, out);
    EOE_CHECK_LAUNCH(who);
    return 0;
}

GridSrc source(int form, const void* base, int64_t n_src, int C, int h, int w) {
    GridSrc s;
    memset(&s, 0, sizeof(s));
    s.form = form, s.base = base, s.n_src = n_src, s.C = C, s.h = h, s.w = w;
    return s;
}

}  // namespace

extern "C" int eoe_grid_f32(const float* x, int64_t n_src, int C, int h, int w, const int32_t* table, int n, int groups, int nrow, int pad,
                            int maxres, int sep_height, int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes,
                            void* stream) {
    return compose("grid_f32", source(GR_F32, x, n_src, C, h, w), table, n, groups, nrow, pad, maxres, sep_height, sep_at, marked, minmax,
                   out, out_bytes, stream);
}

extern "C" int eoe_grid_u8(const uint8_t* set, int64_t n_src, int H, int W, int C, const int32_t* table, int n, int groups, int nrow,
                           int pad, int maxres, int sep_height, int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes,
                           void* stream) {
    return compose("grid_u8", source(GR_U8, set, n_src, C, H, W), table, n, groups, nrow, pad, maxres, sep_height, sep_at, marked, minmax,
                   out, out_bytes, stream);
}

extern "C" int eoe_grid_ragged_u8(const uint8_t* arena, int64_t arena_bytes, const int64_t* offsets, const int32_t* sizes, int64_t n_src,
                                  int C, int crop_h, int crop_w, const int32_t* table, int n, int groups, int nrow, int pad, int maxres,
                                  int sep_height, int sep_at, int marked, float* minmax, uint8_t* out, int64_t out_bytes, void* stream) {
    EOE_CHECK_ARG(n == 0 || (offsets && sizes && arena_bytes > 0), "grid_ragged_u8: null offsets or sizes, or an empty arena");
    GridSrc s = source(GR_RAGGED, arena, n_src, C, crop_h, crop_w);
    s.offsets = (const long long*)offsets, s.sizes = (const int*)sizes, s.arena_bytes = arena_bytes;
    return compose("grid_ragged_u8", s, table, n, groups, nrow, pad, maxres, sep_height, sep_at, marked, minmax, out, out_bytes, stream);
}
