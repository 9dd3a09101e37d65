// The fragment layer of the attention kernels (attention.hip, attention_long.hip, clip_text.hip): the LDS operand image and its
// address contract, the bounds-checked global loads, the MFMA operand fragments read from either, the lane-group reductions, the
// 16-byte row store.  v_mfma_f32_16x16x32_{f16,bf16};
// scores are computed TRANSPOSED (key on the accumulator row = register index, query on the lane), so a product's result is already
// the B operand of the next one (acc_as_operand) with the k order inside a 32-row step permuted to (j < 4: row 32 s + 4 g + j,
// j >= 4: row 32 s + 16 + 4 g + j - 4), which the other operand reproduces by choosing which 4-row blocks its transposing reads fetch.
// Every file pulls this in with `using namespace attn_frag` inside its anonymous namespace.  The kernels' machine code is sensitive to
// the order in which these bodies emit their address arithmetic (register allocation follows it): compare the device assembly of all
// three files before and after a change that is meant to leave them alone.
#pragma once
#include "common.h"

namespace attn_frag {

// ------------------------------------------------------------------------------------------------ the LDS image
constexpr int ROWB = 160;            // LDS row pitch in bytes (64 x 16-bit + pad): conflict-free transposed reads
constexpr int TILEB = 64 * ROWB;     // one 64 x 64 operand image
// (round 5) The 16-byte chunks of ODD rows are stored pairwise swapped (in-row byte offset ^ 16).  With the hardware's lane groups (a
// ds_read_b64_tr_b16 is served in two groups of 32 lanes, banks (a / 4) mod 64) the interleaved transposing read tfrag_il -- dword 40 row + 8 p +
// 2 tc over rows 0-7 x p 0-3 -- put 32 lanes on 16 banks FOUR ways (8 LDS cycles for an ideal 2; attn_bwd4: SQ_LDS_BANK_CONFLICT 3.56 M cycles
// per launch); with the swap two ways, the floor for 8-byte pieces of 16-byte-aligned rows (searched by simulation over every GF(2)-linear
// 3-bit function of the row, pitches 128 / 160 / 192); the ds_read_b128 fragment reads and the plain transposing reads stay conflict-free.
// attn_bwd 0.480 -> 0.465 ms per step, step 10.256 -> 10.222 (three interleaved pairs, tools/cflags_ab.sh -DEOE_ATTN_NO_RSWZ).  Also measured: an
// unpadded 128-byte pitch with the 3-bit term ((row >> 1 & 1) * 3 | row & 4) -- the same conflict profile, 28 KB of LDS per attn_bwd4 workgroup --
// and five workgroups per CU (amdgpu_waves_per_eu(5, 5): 96 registers, 4 spilled): attn_bwd 0.465 -> 0.509 ms per step; not kept.
#ifdef EOE_ATTN_NO_RSWZ          // A/B builds (tools/cflags_ab.sh): the round-4 image, in every attention kernel
__device__ __forceinline__ int rswz(int) { return 0; }
#else
__device__ __forceinline__ int rswz(int row) { return (row & 1) << 4; }
#endif
// THE address contract: the 16-byte chunk ch of row `row` lies at byte row * ROWB + ((ch * 16) ^ rswz(row)).  The readers are lfrag and
// tread below; the writers (grep "rswz(") spell the same expression where they stage.

// ------------------------------------------------------------------------------------------------ global loads
// Loads behind `row < L` branches become load -> s_waitcnt vmcnt(0) -> use, a chain of dependent HBM round trips (round 4: attn_fwd's ISA
// showed eight load/wait/ds_write groups for V alone).  These read through a buffer resource that covers the (image, head) slab; a
// row >= L gets an out-of-range offset, which reads zeros, so the loads are unconditional and a whole batch is in flight before the
// first wait.
__device__ __forceinline__ u32x4 bload16(__amdgpu_buffer_rsrc_t r, int row, int L, unsigned pitchb, unsigned cb) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(row < L ? (unsigned)row * pitchb + cb : EOE_OOB), 0, 0));
}
// one resource over Lb rows of a sequence's packed Q | K | V (rows of ld = 3 D elements), rooted at a head's Q slice: the last row ends
// behind V's 64 columns
__device__ __forceinline__ __amdgpu_buffer_rsrc_t qkv_rsrc(const void* q_row0, int Lb, int ld, int D) {
    return make_rsrc(q_row0, ((unsigned)(Lb - 1) * (unsigned)ld + 2u * (unsigned)D + 64u) * 2u);
}

// ------------------------------------------------------------------------------------------------ operand fragments
template <typename T> using V8 = typename T16<T>::v8;

// row-major fragment of one row per lane (operand element j <-> column 8 * (lane >> 4) + j of k-step ks), zeros for row >= L; cb0 = byte
// offset of the operand's head slice inside a row.  bfrag: 16-row tile t, row 16 t + (lane & 15)
template <typename T>
__device__ __forceinline__ V8<T> rowfrag(__amdgpu_buffer_rsrc_t r, unsigned pitchb, unsigned cb0, int L, int row, int ks, int lane) {
    return __builtin_bit_cast(V8<T>, bload16(r, row, L, pitchb, cb0 + (unsigned)(ks * 4 + (lane >> 4)) * 16u));
}
template <typename T>
__device__ __forceinline__ V8<T> bfrag(__amdgpu_buffer_rsrc_t r, unsigned pitchb, unsigned cb0, int L, int t, int ks, int lane) {
    return rowfrag<T>(r, pitchb, cb0, L, t * 16 + (lane & 15), ks, lane);
}
// the same fragment of tile t from an LDS image
template <typename T>
__device__ __forceinline__ V8<T> lfrag(const char* lds, int t, int ks, int lane) {
    const int row = t * 16 + (lane & 15);
    return __builtin_bit_cast(V8<T>, *(const u32x4*)(lds + row * ROWB + (((ks * 4 + (lane >> 4)) * 16) ^ rswz(row))));
}
// transposed fragments: element j <-> row perm(s, lane >> 4, j) (file header); the lane's first column is CT tc + CP (lane & 3).
// tfrag (CP 4, CT 16): lane <-> column 16 tc + (lane & 15).
// tfrag_il (CP 16, CT 4): the COLUMNS of the four tiles tc = 0..3 interleaved, lane <-> column 16 ((lane & 15) >> 2) + 4 tc + (lane & 3).  As the
// A operand of a transposed product (rows of the result = these columns) it leaves lane (lane & 15, g = lane >> 4) of result tile tc with
// rows 16 g + 4 tc + 0..3 -- over the four tiles 16 CONSECUTIVE rows per lane: a lane's share of an output row is one 32-byte run
// (store_row16) instead of four 8-byte pieces 32 bytes apart.  Only the address each lane hands the transposing read changes.
template <typename T, int CP, int CT>
__device__ __forceinline__ V8<T> tread(const char* lds, int tc, int s, int lane) {
    const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const char* a = lds + (32 * s + 4 * g + q) * ROWB + (((CP * p + CT * tc) * 2) ^ rswz(4 * g + q));
    i16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4v*)(a));
    i16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4v*)(a + 16 * ROWB));
    i16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return __builtin_bit_cast(V8<T>, r);
}
template <typename T>
__device__ __forceinline__ V8<T> tfrag(const char* lds, int tc, int s, int lane) { return tread<T, 4, 16>(lds, tc, s, lane); }
template <typename T>
__device__ __forceinline__ V8<T> tfrag_il(const char* lds, int tc, int s, int lane) { return tread<T, 16, 4>(lds, tc, s, lane); }
// two accumulator tiles (rows 32 s + 0..15 and 32 s + 16..31 of a transposed product) as the next B operand: the 16-bit rounding
template <typename T>
__device__ __forceinline__ V8<T> acc_as_operand(const f32x4& lo, const f32x4& hi) {
    V8<T> r;
    r[0] = (T)lo[0]; r[1] = (T)lo[1]; r[2] = (T)lo[2]; r[3] = (T)lo[3];
    r[4] = (T)hi[0]; r[5] = (T)hi[1]; r[6] = (T)hi[2]; r[7] = (T)hi[3];
    return r;
}
// a lane's 16 consecutive columns of an output row (four packed tiles of a tfrag_il product): two 16-byte stores
template <typename T>
__device__ __forceinline__ void store_row16(T* d, const u32x2 (&pk)[4]) {
    *(u32x4*)d = (u32x4){pk[0][0], pk[0][1], pk[1][0], pk[1][1]};
    *(u32x4*)(d + 8) = (u32x4){pk[2][0], pk[2][1], pk[3][0], pk[3][1]};
}

// ------------------------------------------------------------------------------------------------ reductions
__device__ __forceinline__ float group_max(float v) {   // over the 4 lanes sharing lane & 15
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
// sum over the 16 lanes sharing lane >> 4, in every one of them.  They are one DPP row: quad xor 1, quad xor 2, half-row mirror (quads
// 0<->1, 2<->3 hold equal sums by then), row mirror -- four VALU instructions per value instead of four ds_bpermute round trips
__device__ __forceinline__ f32x4 row16_sum(f32x4 t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = t[r];
        v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
        v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
        v += dpp_mov<0x141>(v);     // row_half_mirror
        v += dpp_mov<0x140>(v);     // row_mirror
        t[r] = v;
    }
    return t;
}
// column sums over the 16 tokens of one accumulator tile (token = lane & 15)
__device__ __forceinline__ f32x4 slab_sum(const f32x4& o, bool valid) { return row16_sum(valid ? o : (f32x4){0.f, 0.f, 0.f, 0.f}); }

}  // namespace attn_frag
