// tn_gemm.h -- what the weight-gradient kernels share (wgrad_bf16, wgradT_bf16, wgrad_tap_bf16, wgrad_tap_x3, wgrad_halo_bf16, the
// all-taps kernel of x3.hip and conv_first).  Each is a "TN" GEMM over pixels: both operands sit pixel-major ([pixel][channel]) in LDS, the
// K-major MFMA fragments come from the transposing LDS read ds_read_b64_tr_b16 (4 rows x 16 columns per 16-lane group, delivered
// column-major), blocks are renumbered so that one pixel slice stays on one XCD and pixels are decomposed with a float
// reciprocal.  The index helpers are __host__ __device__: a CPU program checks
// them over their whole domain (tests/host/tn_index_check.hip).
#pragma once
#include "common.h"

namespace ustrun {

// ---- fragments -------------------------------------------------------------------------------------------------------------------
template <typename E> using frag8 = E __attribute__((ext_vector_type(8)));

// two transposing reads (pixel rows r and r + 4 of a 16-deep step) joined into one MFMA operand of element type E.  The read moves
// 16-bit lanes whatever they hold: the i16 form of the builtin, reinterpreted.
template <typename E = elt_t> __device__ __forceinline__ frag8<E> tr_pair(const char* p0, const char* p1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
    return __builtin_bit_cast(frag8<E>, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// 64-byte segments of a row of RB bytes are XOR-permuted by the row index so that the 4 rows of a transposed read fall on different
// bank segments (256-byte rows: 4 segments, row & 3; 128-byte rows: 2 segments, (row >> 1) & 1)
template <int RB> __device__ __forceinline__ int seg_swz(int row) { return RB >= 256 ? (row & 3) : ((row >> 1) & 1); }

// swizzled tile: rows k0 + 8*(l>>5) + {0..3 | 4..7}, columns col0 + 16*((l>>4)&1) + 4*(l&3) .. +3, delivered column-major
template <int RB, typename E = elt_t> __device__ __forceinline__ frag8<E> tr_frag(const char* tile, int k0, int col0, int lane) {
    const int q = (lane & 15) >> 2, p = lane & 3;
    const int colb = (col0 + 16 * ((lane >> 4) & 1) + 4 * p) * 2;
    const int r0 = k0 + 8 * (lane >> 5) + q, r1 = r0 + 4;
    return tr_pair<E>(tile + r0 * RB + (colb ^ (seg_swz<RB>(r0) << 6)), tile + r1 * RB + (colb ^ (seg_swz<RB>(r1) << 6)));
}

// un-swizzled (padded or half-swapped) tile: lane_base = the lane's own byte offset ((8*(l>>5) + q) * RB + column bytes, any swap
// folded in by the caller), k0 = first pixel row of the fragment
template <int RB, typename E = elt_t> __device__ __forceinline__ frag8<E> tr_frag_rows(const char* lane_base, int k0) {
    return tr_pair<E>(lane_base + k0 * RB, lane_base + (k0 + 4) * RB);
}

// ---- index arithmetic ------------------------------------------------------------------------------------------------------------
// v / d and the remainder for 0 <= v < 2^24 through the float reciprocal invd = 1.f / d (two fix-up steps make it exact)
__host__ __device__ __forceinline__ int fdiv(int v, int d, float invd, int& rem) {
    int q = (int)(((float)v + 0.5f) * invd);
    int r = v - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
    rem = r;
    return q;
}

// (x + inc) mod W for 0 <= x < W < 2^15, 0 <= inc <= 64
__host__ __device__ __forceinline__ int wrap_add(int x, int inc, int W, float invW) {
    const int v = x + inc;
    const int q = (int)(((float)v + 0.5f) * invW);
    int r = v - q * W;
    if (r < 0) r += W;
    if (r >= W) r -= W;
    return r;
}

// Where a block's next tile lies, for the kernels that walk a range of tiles of a batch cut into tiles_y x tiles_x tiles of TH x TW
// pixels per image: (image, first row, first column), wave-uniform, stepped without a division.  Tiles of an image are walked
// DOWN its columns (y fastest): the two dY halo rows a tile shares with the next one are in L2 when that tile asks for them
// (walking along x left them a whole tile row = MBs of other blocks' traffic apart, and every halo row came from memory twice:
// 25 % on top of dY; the halo columns now re-read instead are 12.5 %).  k advances from seek(t) give seek(t + k)
// (tests/host/tn_index_check.hip).
template <int TH, int TW> struct tile_cursor {
    int img, y0, x0, yend, xend;
    __host__ __device__ __forceinline__ void seek(int t, int tiles_y, int tiles_x) {
        img = t / (tiles_y * tiles_x);
        const int rem = t - img * tiles_y * tiles_x;
        x0 = (rem / tiles_y) * TW; y0 = (rem % tiles_y) * TH;
        yend = tiles_y * TH; xend = tiles_x * TW;
    }
    __host__ __device__ __forceinline__ void advance() {
        y0 += TH;
        if (y0 >= yend) {
            y0 = 0; x0 += TW;
            if (x0 >= xend) { x0 = 0; ++img; }
        }
    }
};

// ---- all-taps slab (wgrad_halo_bf16, the all-taps kernel of x3.hip) -------------------------------------------------------------
// A wave's nine 32x32 accumulators D[co][ci] -> the f32 slab in the torch weight layout [Cout][Cin][3][3]: rows of D are co
// (co_base + the MFMA's row of register r), lanes are ci, and a lane holds all nine taps of its (co, ci) pairs -> nine
// consecutive floats.  ADD: partner holds a second set of accumulators as [tap][r][pstride floats], added on the way out.
template <bool ADD = false>
__device__ __forceinline__ void store_slab_oihw9(float* slab, int Cin, int ci, int co_lane, const f32x16 (&acc)[9],
                                                 const float* partner = nullptr, int pstride = 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co_lane + (r & 3) + 8 * (r >> 2);
        float* o = slab + ((long)co * Cin + ci) * 9;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) o[tap] = ADD ? acc[tap][r] + partner[(tap * 16 + r) * pstride] : acc[tap][r];
    }
}

// ---- the one-tap-per-block kernels (wgrad_tap_bf16, wgrad_tap_x3), host side ----------------------------------------------------
// the tile of a problem, and the split-K plan for stages of KP pixels -- at most one resident round of blocks (2 per
// CU), at least four stages per block
inline int tap_tile_m(const WgradArgs& a) { return a.Cin % 128 == 0 ? 128 : 64; }
inline int tap_tile_n(const WgradArgs& a) { return a.Cout % 128 == 0 ? 128 : 64; }
inline int tap_plan(const WgradArgs& a, int KP, int* ksplit, long* kchunk) {
    const long tiles = (long)(a.Cin / tap_tile_m(a)) * (a.Cout / tap_tile_n(a)) * a.nseg;
    long ks = 512 / tiles;                 // rounded DOWN: 36 tiles x 15 slices = 540 blocks ran as 512 + a second round of 28
                                           // (0.21 ms for a 0.11 ms job); 14 slices = 504 blocks finish in one round
    if (ks > a.M / (4 * KP)) ks = a.M / (4 * KP);
    if (ks < 1) ks = 1;
    long chunk = (a.M + ks - 1) / ks;
    chunk = (chunk + KP - 1) / KP * KP;
    *kchunk = chunk; *ksplit = (int)((a.M + chunk - 1) / chunk);
    return 0;
}

}  // namespace ustrun
