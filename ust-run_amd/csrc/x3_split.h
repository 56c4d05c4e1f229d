// x3_split.h -- what the kernels of dtype USTRUN_F32X3 share (x3.hip, wgrad_tap_x3.hip, conv_first.hip): an f32 value as three bf16
// terms, a product of two such values as six bf16 MFMAs with f32 accumulation (see x3.hip's header), and the staging around them:
// the split and its plane stores, the activation, the product schedule, the weight-plane layout, the source state, the host checks.
#pragma once
#include "common.h"
#include "loader.h"         // pick_src, relu4

namespace ustrun {
namespace {

#define X3_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16

// three bf16 terms of four f32 values, each plane as two dwords (four bf16)
__device__ __forceinline__ void split4(const f32x4 v, u32x2& p0, u32x2& p1, u32x2& p2) {
    b16x4 h0, h1, h2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        h0[q] = (__bf16)v[q];
        const float r1 = v[q] - (float)h0[q];          // exact: the low 16 bits of v (+ the rounding carry)
        h1[q] = (__bf16)r1;
        const float r2 = r1 - (float)h1[q];            // exact
        h2[q] = (__bf16)r2;
    }
    p0 = __builtin_bit_cast(u32x2, h0); p1 = __builtin_bit_cast(u32x2, h1); p2 = __builtin_bit_cast(u32x2, h2);
}
// ... as a value, and stored as the three planes of an LDS tile, `plane` bytes apart: store_planes(split3(v), dst, plane).  The
// split is the FIRST argument so that it is formed before the address: the other order changes how hipcc schedules the stores.
struct X3Planes { u32x2 p[3]; };
__device__ __forceinline__ X3Planes split3(const f32x4 v) { X3Planes r; split4(v, r.p[0], r.p[1], r.p[2]); return r; }
__device__ __forceinline__ void store_planes(const X3Planes& r, char* dst, int plane) {
    *(u32x2*)dst = r.p[0]; *(u32x2*)(dst + plane) = r.p[1]; *(u32x2*)(dst + 2 * plane) = r.p[2];
}

// A staged activation: BatchNorm affine and ReLU in f32, then zero where the item lies outside the image (padding is applied AFTER
// the activation).  Two spellings of the ReLU, chosen at compile time and NOT unified: relu4 (v_med3_f32) and fmaxf (a canonicalising
// v_max_f32) may differ in the sign of a zero and in the NaN they return, and every kernel keeps the bits it had.  FLOOR = false
// (forward, input gradient, ConvTranspose weight gradient): `act` is the source's relu flag, relu4 under a branch.  FLOOR = true
// (the other weight gradients): `act` is x3_floor(relu), formed once per kernel, branch-free fmaxf.
__device__ __forceinline__ float x3_floor(int relu) { return relu ? 0.f : -__builtin_inff(); }
template <bool FLOOR, typename T>
__device__ __forceinline__ f32x4 x3_activate(const f32x4 raw, const f32x4 sc, const f32x4 sh, T act, bool ok) {
    f32x4 v = raw * sc + sh;
    if constexpr (FLOOR) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __builtin_fmaxf(v[q], act);
    } else {
        if (act) v = relu4(v);
    }
    if (!ok) v = (f32x4){0.f, 0.f, 0.f, 0.f};
    return v;
}

// ---- the product schedule: a b ~ a0 b2 + a1 b1 + a2 b0 + a0 b1 + a1 b0 + a0 b0, small terms first -------------------------------
constexpr int X3_TA[6] = {0, 1, 2, 0, 1, 0}, X3_TB[6] = {2, 1, 0, 1, 0, 0};

// one fragment pair, one accumulator: the six MFMAs back to back
__device__ __forceinline__ f32x16 mfma6(const b16x8 (&a)[3], const b16x8 (&b)[3], f32x16 c) {
#pragma unroll
    for (int q = 0; q < 6; ++q) c = X3_MFMA(a[X3_TA[q]], b[X3_TB[q]], c, 0, 0, 0);
    return c;
}
// MI x NI accumulators, term by term over all of them: the six products of one accumulator stand MI * NI instructions apart, in
// mfma6's order whatever the walk.  J_OUTER: columns outer (each kernel keeps its issue order).  SWAP: the operands trade places
// (D = b^T a: the 1x1 weight-gradient slab layout).  BT: b16x8, or the u32x4 a fragment was loaded as.
template <bool J_OUTER, bool SWAP, int MI, int NI, typename BT>
__device__ __forceinline__ void x3_products(const b16x8 (&a)[MI][3], const BT (&b)[NI][3], f32x16 (&acc)[MI][NI]) {
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int o = 0; o < (J_OUTER ? NI : MI); ++o)
#pragma unroll
            for (int n = 0; n < (J_OUTER ? MI : NI); ++n) {
                const int i = J_OUTER ? n : o, j = J_OUTER ? o : n;
                const b16x8 bq = __builtin_bit_cast(b16x8, b[j][X3_TB[q]]);
                acc[i][j] = SWAP ? X3_MFMA(bq, a[i][X3_TA[q]], acc[i][j], 0, 0, 0) : X3_MFMA(a[i][X3_TA[q]], bq, acc[i][j], 0, 0, 0);
            }
}

// ---- packed weight planes: f32 [S][K][N] -> bf16 [S][3][K/8][N][8], which IS the B-fragment layout ------------------------------
// element offset of the eight consecutive k of (k8, n) inside a plane: the pack kernel writes there, the fragment loads read there.
// (The plane size (long)(K / 8) * N * 8 and the fragment loop of x3.hip's load_b lambdas stay at their sites: as functions of this
// header they change the device code of pack_x3, igemm_x3 and conv3x3_x3 -- profiles/x3_shared_ab.log, item 1.)
__host__ __device__ constexpr long x3_woff(long k8, long n, long N) { return (k8 * N + n) * 8; }

// ---- the source a channel chunk is staged from ------------------------------------------------------------------------------------
// ptr / relu / cbase (its first channel inside the concatenation) of the first or second source, scale / shift ALREADY offset for the
// pass of image `img` (gN images per pass, gstride floats apart: a tile is split with the constants of its own image).  select
// returns the picked source for the caller's geometry.
struct X3Src {
    const float *ptr, *scale, *shift;
    int relu, cbase;
    template <typename Args>
    __device__ __forceinline__ SrcDev select(const Args& a, bool second, int img) {
        const SrcDev S = pick_src(a.src[0], a.src[1], second);
        const long gofs = (S.scale && S.gN > 0) ? (long)(img / S.gN) * S.gstride : 0;
        ptr = S.ptr; scale = S.scale ? S.scale + gofs : nullptr; shift = S.shift ? S.shift + gofs : nullptr; relu = S.relu;
        cbase = second ? a.src[0].C : 0;
        return S;
    }
    // the constants of channels cl .. cl + 3 of this source (the identity without BatchNorm)
    __device__ __forceinline__ void consts(int cl, f32x4& sc, f32x4& sh) const {
        sc = (f32x4){1.f, 1.f, 1.f, 1.f}; sh = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (scale) { sc = *(const f32x4*)(scale + cl); sh = *(const f32x4*)(shift + cl); }
    }
};

// ---- host side ----------------------------------------------------------------------------------------------------------------
// what every f32x3 kernel asks of a source: f32, channels contiguous, 16-byte loads of four channels, no pooling on load
static inline bool x3_src_ok(const SrcDev& s) {
    return s.esz == 4 && s.sC == 1 && !(s.C & 3) && !s.pool && !((s.sN | s.sH | s.sW) & 3);
}
// split-K over space for the all-taps weight gradients: about one block per CU (256 over the ci x co tile pairs), no block with
// fewer than min_tiles spatial tiles; slabs == ksplit
static inline void space_split_plan(long pairs, int tiles_total, int min_tiles, int* ksplit, int* tiles_per) {
    long ks = (256 + pairs - 1) / pairs;
    if (ks > tiles_total / min_tiles) ks = tiles_total / min_tiles;
    if (ks < 1) ks = 1;
    const int per = cdiv(tiles_total, ks);
    *tiles_per = per; *ksplit = cdiv(tiles_total, per);
}

}  // namespace
}  // namespace ustrun
