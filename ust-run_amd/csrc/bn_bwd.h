// BatchNorm (+ ReLU, + MaxPool routing) backward: the kernels of bn.hip's three stream passes -- reduce, apply, frozen -- and of
// the finalize between them.  Each lane width has ONE stream body (bn_bwd_stream4, bn_bwd_stream8); the __global__ kernels are
// wrappers that name a pass.
#pragma once
#include <type_traits>

#include "common.h"
#include "loader.h"

namespace ustrun {
namespace {

// One "window" = one pixel (POOL = false) or one 2x2 pooling window (POOL = true).  For each
// element: a = relu(s*y+b); da_total = da + (dp routed to the window's first arg-max of a);
// dz = da_total * (a > 0).  Returns the offset of the window's first pixel (channel c): the stores of a pass start from it.
//
// EVEN (pooled windows of an even-sized map: every U-Net level): all four pixels and the pooled cell exist, so the validity
// selects (3 per element), the clamped addresses and the integer arg-max index go away -- the routing is three compares per channel
// and mask logic.  The general form below costs 360 VALU instructions per window for 72 loaded bytes: the pooled reduce was issue
// bound at 3.3 TB/s (profiles/r03_bench_bn_bwd.log).
template <bool POOL, int ESZ, bool EVEN = false>
__device__ __forceinline__ long window_dz(const float* da, const float* __restrict__ dp, const float* __restrict__ y, f32x4 sc,
                                          f32x4 sh, long w, int WH, int WW, int H, int W, int C, int c, f32x4 (&yv)[POOL ? 4 : 1],
                                          f32x4 (&dz)[POOL ? 4 : 1], bool (&ok)[POOL ? 4 : 1]) {
    constexpr int NPX = POOL ? 4 : 1;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 av[NPX];
    if constexpr (POOL && EVEN) {
        const unsigned uw = (unsigned)w, per = (unsigned)(WH * WW);
        const unsigned n = uw / per, rem = uw - n * per, wy = rem / (unsigned)WW, wx = rem - wy * (unsigned)WW;
        const long off0 = (((long)n * H + 2 * wy) * W + 2 * wx) * C + c;
        const long rowo = (long)W * C;
        yv[0] = ld4t<ESZ>(y, off0); yv[1] = ld4t<ESZ>(y, off0 + C); yv[2] = ld4t<ESZ>(y, off0 + rowo); yv[3] = ld4t<ESZ>(y, off0 + rowo + C);
        if (da) {
            dz[0] = ld4t<ESZ>(da, off0); dz[1] = ld4t<ESZ>(da, off0 + C); dz[2] = ld4t<ESZ>(da, off0 + rowo); dz[3] = ld4t<ESZ>(da, off0 + rowo + C);
        } else {
            dz[0] = dz[1] = dz[2] = dz[3] = zero;
        }
        const f32x4 g4 = dp ? ld4t<ESZ>(dp, (long)w * C + c) : zero;       // the pooled map's cell IS window w
#pragma unroll
        for (int q = 0; q < 4; ++q) { ok[q] = true; av[q] = yv[q] * sc + sh; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // first arg-max of relu(a) in the order (0,0) (0,1) (1,0) (1,1): strict > keeps the first
            const float a0 = fmaxf(av[0][j], 0.f), a1 = fmaxf(av[1][j], 0.f), a2 = fmaxf(av[2][j], 0.f), a3 = fmaxf(av[3][j], 0.f);
            const bool m1 = a1 > a0;
            const float b1 = fmaxf(a0, a1);
            const bool m2 = a2 > b1;
            const float b2 = fmaxf(b1, a2);
            const bool m3 = a3 > b2;
            const float g = g4[j];
            const bool e3 = m3, e2 = m2 && !m3, e1 = m1 && !m2 && !m3, e0 = !(m1 || m2 || m3);
            dz[0][j] += e0 ? g : 0.f; dz[1][j] += e1 ? g : 0.f; dz[2][j] += e2 ? g : 0.f; dz[3][j] += e3 ? g : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) dz[q][j] = (av[q][j] > 0.f) ? dz[q][j] : 0.f;
        return off0;
    }
    // plain: the window IS the pixel, its offset is linear (no division: these kernels were instruction bound on the
    // 64-bit divides, not memory bound); pooled: 32-bit divides (windows per pass < 2^31)
    int n = 0, wy = 0, wx = 0;
    if (POOL) {
        const unsigned uw = (unsigned)w, per = (unsigned)(WH * WW);
        n = (int)(uw / per);
        const unsigned rem = uw - (unsigned)n * per;
        wy = (int)(rem / (unsigned)WW); wx = (int)(rem - (unsigned)wy * (unsigned)WW);
    }
    // every load of the window is issued unconditionally (out-of-range pixels read the window's first pixel, always
    // inside, and are zeroed afterwards): nine independent loads in flight instead of one masked region after another
    const long off0 = POOL ? (((long)n * H + 2 * wy) * W + 2 * wx) * C + c : w * C + c;
#pragma unroll
    for (int q = 0; q < NPX; ++q) {
        const int py = 2 * wy + (q >> 1), px = 2 * wx + (q & 1);
        ok[q] = !POOL || (py < H && px < W);
        const long off = ok[q] ? off0 + ((long)(q >> 1) * W + (q & 1)) * C : off0;
        yv[q] = ld4t<ESZ>(y, off);
        if constexpr (POOL) dz[q] = da ? ld4t<ESZ>(da, off) : zero;      // (pooled layers may have no direct consumer)
        else dz[q] = ld4t<ESZ>(da, off);                                  // plain: da is always there -- no branch around the load
    }
    f32x4 gpool = zero;
    bool gok = false;
    if (POOL && dp) {
        const int PH = H / 2, PW = W / 2;
        gok = wy < PH && wx < PW;
        gpool = ld4t<ESZ>(dp, (((long)n * PH + (gok ? wy : 0)) * PW + (gok ? wx : 0)) * C + c);
    }
    // everything below is selects, not branches (the compiler turned the arg-max routing into ~40 exec-mask regions)
#pragma unroll
    for (int q = 0; q < NPX; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            yv[q][j] = ok[q] ? yv[q][j] : 0.f;
            dz[q][j] = ok[q] ? dz[q][j] : 0.f;
            av[q][j] = ok[q] ? yv[q][j] * sc[j] + sh[j] : 0.f;
        }
    }
    if (POOL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = gok ? gpool[j] : 0.f;
            // first arg-max of relu(a) over the window, in the order (0,0) (0,1) (1,0) (1,1): strict > keeps the first
            const float a0 = fmaxf(av[0][j], 0.f), a1 = fmaxf(av[1][j], 0.f), a2 = fmaxf(av[2][j], 0.f), a3 = fmaxf(av[3][j], 0.f);
            const bool m1 = a1 > a0;
            const float b1 = m1 ? a1 : a0;
            const bool m2 = a2 > b1;
            const float b2 = m2 ? a2 : b1;
            const bool m3 = a3 > b2;
            const int best = m3 ? 3 : (m2 ? 2 : (m1 ? 1 : 0));
#pragma unroll
            for (int q = 0; q < NPX; ++q) dz[q][j] += (q == best) ? g : 0.f;
        }
    }
#pragma unroll
    for (int q = 0; q < NPX; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) dz[q][j] = (av[q][j] > 0.f) ? dz[q][j] : 0.f;
    return off0;
}

// blockIdx.y = forward pass (batched passes: each has its own slice of every tensor, constants, partial rows and coefficients)
struct PassOff { long act, pool, aff, part, coef; };   // element strides between passes (bytes are esz * act for tensors)

// the calling block's pass of an array whose passes lie `elems` elements of ESZ bytes apart
template <int ESZ, typename T>
__device__ __forceinline__ T* pass_of(T* p, long elems) {
    return (T*)((char*)p + (long)blockIdx.y * elems * ESZ);
}

// The end of a pass that forms sums: a lane's {s1, s2} (NV f32x4 each: NV * 4 channels from c on) and those of the block's other
// pixel lanes of the same channel group g, added in ascending lane order, are the block's partial row partials[block][2][C].
// Thread = (group tid % G, pixel lane tid / G).  Holds a barrier: every thread of the block calls it.  The LDS belongs to this
// function, so a kernel that forms no sums allocates none.
template <int NV>
__device__ __forceinline__ void block_fold(f32x4 (&s1)[NV], f32x4 (&s2)[NV], int G, int g, int pl, bool active,
                                           float* __restrict__ partials, int C, int c) {
    __shared__ f32x4 red[2 * NV][256];
#pragma unroll
    for (int v = 0; v < NV; ++v) { red[v][threadIdx.x] = s1[v]; red[NV + v][threadIdx.x] = s2[v]; }
    __syncthreads();
    if (pl == 0 && active) {
        const int PL = 256 / G;
        for (int k = 1; k < PL; ++k) {
#pragma unroll
            for (int v = 0; v < NV; ++v) { s1[v] += red[v][k * G + g]; s2[v] += red[NV + v][k * G + g]; }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            *(f32x4*)(partials + ((long)blockIdx.x * 2 + 0) * C + c + 4 * v) = s1[v];
            *(f32x4*)(partials + ((long)blockIdx.x * 2 + 1) * C + c + 4 * v) = s2[v];
        }
    }
}

// The apply pass's dy = k0 dz + k1 y + k2 in the operations every build of it has used: one product rounded, the other fused onto
// it, then + k2.  Left to hipcc's contraction, WHICH product is rounded depends on how the loop around the statement is scheduled:
// the pooled builds have always rounded k1 y, the plain ones k0 dz.
template <bool POOL>
__device__ __forceinline__ f32x4 bn_bwd_dy4(f32x4 k0, f32x4 k1, f32x4 k2, f32x4 dz, f32x4 yv) {
#pragma clang fp contract(off)
    if constexpr (POOL) return __builtin_elementwise_fma(k0, dz, k1 * yv) + k2;
    else return __builtin_elementwise_fma(k1, yv, k0 * dz) + k2;
}

// The three passes over (da [, dp], y) are one walk: grid-stride over windows, thread = (channel group, window lane), per element
// dz as window_dz forms it.  They differ in what leaves the walk:
//   BN_REDUCE  sums {dz, dz y} per block (block_fold), no store;
//   BN_APPLY   dy = k0 dz + k1 y + k2 (coef[3][C] from the finalize), no sums;
//   BN_FROZEN  dy = scale dz, SUMS: the sums too.
// (the values are the pass codes of ustrun_debug_last_bn_variant)
enum { BN_REDUCE = 0, BN_APPLY = 1, BN_FROZEN = 2 };

// Four channels per lane: every storage type, plain and pooled.  G = the power of two >= C / 4 (at most 256); more than 4 G
// channels take several rounds of the channel loop, whose trip count is uniform (with SUMS the body holds barriers) and in whose
// last round the lanes past C sit idle.
template <bool POOL, int ESZ, bool EVEN, int PASS, bool SUMS>
__device__ __forceinline__ void bn_bwd_stream4(const float* da, const float* dp, const float* y, const float* scale,
                                               const float* shift, const float* coef, int N, int H, int W, int C, int G, float* dy,
                                               float* partials, const PassOff& po) {
    constexpr int NPX = POOL ? 4 : 1;
    // windows per trip.  Reduce, plain: four, their eight loads issued before the first use (one window per trip left the
    // memory-level parallelism to occupancy alone: 4.7 -> 5.2 TB/s; eight per trip: no further gain); the sums still run in
    // ascending window order.  With stores: one -- with four the loads and the four stores of a trip queue behind each other
    // (measured 110 -> 125 us in the apply pass, while the store-free reduce gained 13 % from the same change).
    constexpr int U = (PASS == BN_REDUCE && !POOL) ? 4 : 1;
    if (da) da = pass_of<ESZ>(da, po.act);          // (a null da or dp says: no such term)
    if (dp) dp = pass_of<ESZ>(dp, po.pool);
    y = pass_of<ESZ>(y, po.act); scale = pass_of<4>(scale, po.aff); shift = pass_of<4>(shift, po.aff);
    if constexpr (PASS != BN_REDUCE) dy = pass_of<ESZ>(dy, po.act);
    if constexpr (PASS == BN_APPLY) coef = pass_of<4>(coef, po.coef);
    if constexpr (SUMS) partials = pass_of<4>(partials, po.part);
    const int C4 = C / 4, PL = 256 / G;
    const int cq0 = threadIdx.x % G, pl = threadIdx.x / G;
    const int WH = POOL ? (H + 1) / 2 : H, WW = POOL ? (W + 1) / 2 : W;
    const long nwin = (long)N * WH * WW;
    for (int cb = 0; cb < C4; cb += G) {
        const int cq = cb + cq0;
        const bool active = cq < C4;
        const int c = active ? cq * 4 : 0;
        const f32x4 sc = *(const f32x4*)(scale + c), sh = *(const f32x4*)(shift + c);
        f32x4 k0 = sc, k1 = sc, k2 = sc;
        if constexpr (PASS == BN_APPLY) { k0 = *(const f32x4*)(coef + c); k1 = *(const f32x4*)(coef + C + c); k2 = *(const f32x4*)(coef + 2 * C + c); }
        f32x4 s1[1] = {{0.f, 0.f, 0.f, 0.f}}, s2[1] = {{0.f, 0.f, 0.f, 0.f}};
        auto trip = [&](auto nu, long w, long stride) {          // the windows w, w + stride, ...: all loads, then sums and stores in that order
            constexpr int UU = decltype(nu)::value;
            f32x4 yv[UU][NPX], dz[UU][NPX]; bool ok[UU][NPX]; long base[UU];
#pragma unroll
            for (int u = 0; u < UU; ++u) base[u] = window_dz<POOL, ESZ, EVEN>(da, dp, y, sc, sh, w + u * stride, WH, WW, H, W, C, c, yv[u], dz[u], ok[u]);
#pragma unroll
            for (int u = 0; u < UU; ++u)
#pragma unroll
                for (int q = 0; q < NPX; ++q) {
                    if constexpr (SUMS) { s1[0] += dz[u][q]; s2[0] += dz[u][q] * yv[u][q]; }       // (pixels outside the map carry dz = y = 0)
                    if constexpr (PASS != BN_REDUCE) {
                        if (!ok[u][q]) continue;
                        const long o = base[u] + ((long)(q >> 1) * W + (q & 1)) * C;
                        if constexpr (PASS == BN_APPLY) st4t<ESZ>(dy, o, bn_bwd_dy4<POOL>(k0, k1, k2, dz[u][q], yv[u][q]));
                        else st4t<ESZ>(dy, o, sc * dz[u][q]);    // (in place where dy == da: a thread owns its window's elements, loaded before they are stored)
                    }
                }
        };
        if (active) {
            const long stride = (long)gridDim.x * PL;
            long w = (long)blockIdx.x * PL + pl;
            for (; w + (U - 1) * stride < nwin; w += U * stride) trip(std::integral_constant<int, U>{}, w, stride);
            if constexpr (U > 1)
                for (; w < nwin; w += stride) trip(std::integral_constant<int, 1>{}, w, stride);
        }
        if constexpr (SUMS) {
            block_fold<1>(s1, s2, G, cq0, pl, active, partials, C, c);
            __syncthreads();
        }
    }
}

template <bool POOL, int ESZ, bool EVEN = false>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ da, const float* __restrict__ dp,
                                                           const float* __restrict__ y, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int N, int H, int W, int C,
                                                           int G, float* __restrict__ partials, const PassOff po) {
    bn_bwd_stream4<POOL, ESZ, EVEN, BN_REDUCE, true>(da, dp, y, scale, shift, nullptr, N, H, W, C, G, nullptr, partials, po);
}

template <bool POOL, int ESZ, bool EVEN = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* da, const float* __restrict__ dp,
                                                          const float* __restrict__ y, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ coef,
                                                          int N, int H, int W, int C, int G, float* dy, const PassOff po) {
    bn_bwd_stream4<POOL, ESZ, EVEN, BN_APPLY, false>(da, dp, y, scale, shift, coef, N, H, W, C, G, dy, nullptr, po);
}

// ---- frozen BatchNorm (running statistics): the backward in ONE pass ----------------------------------------------------------
// With scale = gamma rstd and shift = beta - running_mean scale fixed, dy = scale g with g = (da [+ routed dp]) [y scale + shift > 0]
// needs no batch sum: the apply pass does not wait for a reduce pass, and both read the same da, dp and y -- so one kernel reads
// each once, writes dy (in place where dy == da) and, SUMS, leaves the block's row {sum g, sum g y} for bn_bwd_finalize_kernel.
// SUMS = false (frozen parameters): a pure apply pass, no LDS, no row.
template <bool POOL, int ESZ, bool EVEN, bool SUMS>
__global__ __launch_bounds__(256) void bn_bwd_frozen_kernel(const float* da, const float* __restrict__ dp, const float* __restrict__ y,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           int N, int H, int W, int C, int G, float* dy,
                                                           float* __restrict__ partials, const PassOff po) {
    bn_bwd_stream4<POOL, ESZ, EVEN, BN_FROZEN, SUMS>(da, dp, y, scale, shift, nullptr, N, H, W, C, G, dy, partials, po);
}

// ---- plain (un-pooled) bf16 passes with 8 channels = 16 bytes per lane (round 3) --------------------------------------------
// The 4-channel kernels above keep 16 bytes per thread in flight (two 8-byte loads, one pixel per trip in the apply pass): at
// their occupancy that is about half of what 8 TB/s x the memory latency asks of a CU, and the plain apply pass ran at
// 4.8-5.1 TB/s where the pooled one (nine loads per thread) reaches 5.5.  Here a lane owns 8 channels of a pixel: thread =
// (octet tid % G8, pixel lane tid / G8), G8 = C / 8 a power of two <= 256; the arithmetic is the same per element.
// (F8, up8, ld8f and the apply statement bn_bwd_apply8 live in common.h: the first convolution's weight gradient uses them too)
struct Bn8Consts { F8 sc, sh, k0, k1, k2; };
template <bool COEF>
__device__ __forceinline__ Bn8Consts ld_bn8(const float* scale, const float* shift, const float* coef, int C, int c) {
    Bn8Consts k;
    k.sc = ld8f(scale + c); k.sh = ld8f(shift + c);
    if constexpr (COEF) { k.k0 = ld8f(coef + c); k.k1 = ld8f(coef + C + c); k.k2 = ld8f(coef + 2 * C + c); }
    else k.k0 = k.k1 = k.k2 = k.sc;
    return k;
}

// Pixels per trip: four in the store-free reduce (their loads in flight, sums in ascending pixel order), two where a trip stores.
template <int PASS, bool SUMS>
__device__ __forceinline__ void bn_bwd_stream8(const elt_t* da, const elt_t* y, const float* scale, const float* shift,
                                               const float* coef, long npix, int C, int G8, elt_t* dy, float* partials,
                                               const PassOff& po) {
    constexpr int U = PASS == BN_REDUCE ? 4 : 2;
    da = pass_of<sizeof(elt_t)>(da, po.act); y = pass_of<sizeof(elt_t)>(y, po.act);
    scale = pass_of<4>(scale, po.aff); shift = pass_of<4>(shift, po.aff);
    if constexpr (PASS != BN_REDUCE) dy = pass_of<sizeof(elt_t)>(dy, po.act);
    if constexpr (PASS == BN_APPLY) coef = pass_of<4>(coef, po.coef);
    if constexpr (SUMS) partials = pass_of<4>(partials, po.part);
    const int PL = 256 / G8;
    const int g8 = threadIdx.x % G8, c = 8 * g8, pl = threadIdx.x / G8;
    const Bn8Consts k = ld_bn8<PASS == BN_APPLY>(scale, shift, coef, C, c);
    f32x4 s1[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, s2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    auto one = [&](bf16x8 yb, bf16x8 db) {      // one pixel's 8 channels: the sums, and what the pass stores
        if constexpr (PASS == BN_APPLY) return bn_bwd_apply8(yb, db, k.sc, k.sh, k.k0, k.k1, k.k2);
        else {
            const F8 yv = up8(yb), dv = up8(db);
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float al = yv.lo[j] * k.sc.lo[j] + k.sh.lo[j], ah = yv.hi[j] * k.sc.hi[j] + k.sh.hi[j];
                const float zl = al > 0.f ? dv.lo[j] : 0.f, zh = ah > 0.f ? dv.hi[j] : 0.f;
                if constexpr (SUMS) {
                    s1[0][j] += zl; s1[1][j] += zh;
                    s2[0][j] += zl * yv.lo[j]; s2[1][j] += zh * yv.hi[j];
                }
                o[j] = (elt_t)(k.sc.lo[j] * zl); o[4 + j] = (elt_t)(k.sc.hi[j] * zh);
            }
            return o;
        }
    };
    const long stride = (long)gridDim.x * PL;
    long w = (long)blockIdx.x * PL + pl;
    for (; w + (U - 1) * stride < npix; w += U * stride) {
        bf16x8 yb[U], db[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { yb[u] = *(const bf16x8*)(y + (w + u * stride) * C + c); db[u] = *(const bf16x8*)(da + (w + u * stride) * C + c); }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bf16x8 o = one(yb[u], db[u]);
            if constexpr (PASS != BN_REDUCE) *(bf16x8*)(dy + (w + u * stride) * C + c) = o;
        }
    }
    for (; w < npix; w += stride) {
        const bf16x8 o = one(*(const bf16x8*)(y + w * C + c), *(const bf16x8*)(da + w * C + c));
        if constexpr (PASS != BN_REDUCE) *(bf16x8*)(dy + w * C + c) = o;
    }
    if constexpr (SUMS) block_fold<2>(s1, s2, G8, g8, pl, true, partials, C, c);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_x8_kernel(const elt_t* __restrict__ da, const elt_t* __restrict__ y,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ coef, long npix, int C, int G8,
                                                             elt_t* __restrict__ dy, const PassOff po) {
    bn_bwd_stream8<BN_APPLY, false>(da, y, scale, shift, coef, npix, C, G8, dy, nullptr, po);
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_x8_kernel(const elt_t* __restrict__ da, const elt_t* __restrict__ y,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              long npix, int C, int G8, float* __restrict__ partials,
                                                              const PassOff po) {
    bn_bwd_stream8<BN_REDUCE, true>(da, y, scale, shift, nullptr, npix, C, G8, nullptr, partials, po);
}

template <bool SUMS>
__global__ __launch_bounds__(256) void bn_bwd_frozen_x8_kernel(const elt_t* da, const elt_t* __restrict__ y,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              long npix, int C, int G8, elt_t* dy, float* __restrict__ partials,
                                                              const PassOff po) {
    bn_bwd_stream8<BN_FROZEN, SUMS>(da, y, scale, shift, nullptr, npix, C, G8, dy, partials, po);
}

// The apply pass for the layer under the head, whose da nobody stored: da[p][c] = sum_k dl[k][p] w[k][c] is formed again from the K
// f32 values of dl per pixel (8 B at K = 2, against 128 B of stored gradient) exactly as head_bwd_kernel forms it -- head_grad4,
// rounded to the storage type as its store rounds it -- and goes through bn_bwd_apply8 like a loaded one.  dl is NCHW: dl[(n K + k) HW
// + hw]; a trip's first pixel is block-uniform, so the division by HW runs once per trip on the scalar unit and a lane only steps
// over image ends (hence a trip loop of its own).  KT > 0: the class count at compile time; KT == 0: any K <= HEAD_KMAX.
constexpr int HEAD_KMAX = 8;
template <int KT>
__global__ __launch_bounds__(256) void bn_bwd_apply_head_x8_kernel(const float* __restrict__ dl, const float* __restrict__ w_head,
                                                                  const elt_t* __restrict__ y, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, const float* __restrict__ coef,
                                                                  long npix, int HW, int C, int G8, int Krt, elt_t* __restrict__ dy,
                                                                  const PassOff po) {
    constexpr int KN = KT > 0 ? KT : HEAD_KMAX;
    const int K = KT > 0 ? KT : Krt;
    dl = pass_of<4>(dl, npix * K); y = pass_of<sizeof(elt_t)>(y, po.act); dy = pass_of<sizeof(elt_t)>(dy, po.act);
    scale = pass_of<4>(scale, po.aff); shift = pass_of<4>(shift, po.aff); coef = pass_of<4>(coef, po.coef);
    const int PL = 256 / G8;
    const int c = 8 * (threadIdx.x % G8), pl = threadIdx.x / G8;
    const Bn8Consts k8 = ld_bn8<true>(scale, shift, coef, C, c);
    f32x4 wlo[KN], whi[KN];
#pragma unroll
    for (int k = 0; k < KN; ++k) {
        const bool on = KT > 0 || k < K;
        wlo[k] = on ? *(const f32x4*)(w_head + k * C + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        whi[k] = on ? *(const f32x4*)(w_head + k * C + c + 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const long stride = (long)gridDim.x * PL;
    constexpr int U = 2;
    // the K values of dl at pixel wb + pl (wb: the trip's first pixel, block-uniform)
    auto load_d = [&](long wb, float (&d)[KN]) {
        const unsigned n0 = (unsigned)wb / (unsigned)HW;              // npix < 2^31 (checked on the host)
        long n = n0;
        int hw = (int)(wb - (long)n0 * HW) + pl;
        while (hw >= HW) { hw -= HW; ++n; }
        const float* p = dl + n * K * HW + hw;
#pragma unroll
        for (int k = 0; k < KN; ++k) d[k] = (KT > 0 || k < K) ? p[(long)k * HW] : 0.f;
    };
    auto grad = [&](const float (&d)[KN]) {
        const f32x4 lo = head_grad4<KN, KT == 0>(d, wlo, K), hi = head_grad4<KN, KT == 0>(d, whi, K);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j] = (elt_t)lo[j]; o[4 + j] = (elt_t)hi[j]; }
        return o;
    };
    long wb = (long)blockIdx.x * PL;
    for (; wb + pl + (U - 1) * stride < npix; wb += U * stride) {
        bf16x8 yb[U]; float d[U][KN];
#pragma unroll
        for (int u = 0; u < U; ++u) { yb[u] = *(const bf16x8*)(y + (wb + pl + u * stride) * C + c); load_d(wb + u * stride, d[u]); }
#pragma unroll
        for (int u = 0; u < U; ++u)
            *(bf16x8*)(dy + (wb + pl + u * stride) * C + c) = bn_bwd_apply8(yb[u], grad(d[u]), k8.sc, k8.sh, k8.k0, k8.k1, k8.k2);
    }
    for (; wb + pl < npix; wb += stride) {
        float d[KN];
        load_d(wb, d);
        *(bf16x8*)(dy + (wb + pl) * C + c) = bn_bwd_apply8(*(const bf16x8*)(y + (wb + pl) * C + c), grad(d), k8.sc, k8.sh, k8.k0, k8.k1, k8.k2);
    }
}

// partials[pass][rows][2][C] -> dgamma, dbeta (the passes' contributions added one after the other, as separate calls
// would).  COEF: also coef[pass][3][C] for the apply pass.  COEF = false serves frozen BatchNorm: dbeta = sum g, dgamma =
// rstd (sum g y - running_mean sum g) with `mean` the running mean; dy does not depend on the sums, gamma and count are unused.
template <bool PRE, bool COEF = true>
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ partials, int rows, int C, double count,
                                       const float* __restrict__ gamma, const float* __restrict__ mean,
                                       const float* __restrict__ rstd, float* dgamma, float* dbeta, int accumulate,
                                       float* coef, int passes, const PassOff po, long rstride, long roff, int R) {
    __shared__ double red[2][32][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;      // 32 channels x 32 row lanes
    const int c = blockIdx.x * 32 + cl;
    float dg_run = 0.f, db_run = 0.f;
    if (rg == 0 && c < C && dgamma && accumulate) { dg_run = dgamma[c]; db_run = dbeta[c]; }
    // up to four passes per round, eight row lanes each (as bn_finalize_kernel: the passes' sums are independent, only the
    // dgamma/dbeta accumulation is sequential; a pass's sums are formed in the same order alone or batched)
    constexpr int LPP = 8, PPR = 32 / LPP;
    const int gl = rg / LPP, lane = rg % LPP;
    for (int g0 = 0; g0 < passes; g0 += PPR) {
        const int g = g0 + gl;
        double s1 = 0.0, s2 = 0.0;
        if (c < C && g < passes) {
            const float* pt = partials + (long)g * po.part + roff + c;
            if constexpr (PRE) {     // rows of a convolution's epilogue, pre-reduced in place by bn_stat_stage1_kernel: f64 sums parked as
                                     // (hi, lo) float pairs at rows sp*R (sum 1) and sp*R+1 (sum 2); at most 32 splits = four per lane
                float v[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sp = lane + LPP * k;
                    const bool ok = sp * R < rows;
                    const long a0 = ok ? (long)(sp * R) * 2 * C : 0, a1 = ok ? (long)(sp * R + 1) * 2 * C : 0;
                    const float x0 = pt[a0], x1 = pt[a0 + C], x2 = pt[a1], x3 = pt[a1 + C];
                    v[k][0] = ok ? x0 : 0.f; v[k][1] = ok ? x1 : 0.f; v[k][2] = ok ? x2 : 0.f; v[k][3] = ok ? x3 : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) { s1 += (double)v[k][0] + (double)v[k][1]; s2 += (double)v[k][2] + (double)v[k][3]; }
            }
            int r = PRE ? rows : lane;
            for (; r + 7 * LPP < rows; r += 8 * LPP) {       // eight rows' loads issued before the first sum (written out: left
                float a[8], b[8];                            // to the unroller, each load was waited for on its own)
#pragma unroll
                for (int u = 0; u < 8; ++u) { const float* q = pt + (long)(r + u * LPP) * rstride; a[u] = q[0]; b[u] = q[C]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) { s1 += (double)a[u]; s2 += (double)b[u]; }
            }
            for (; r < rows; r += LPP) {
                s1 += (double)pt[(long)r * rstride];
                s2 += (double)pt[(long)r * rstride + C];
            }
        }
        red[0][rg][cl] = s1; red[1][rg][cl] = s2;
        __syncthreads();
        if (rg == 0 && c < C) {
            for (int q = 0; q < PPR && g0 + q < passes; ++q) {
                double t1 = 0.0, t2 = 0.0;
                for (int k = 0; k < LPP; ++k) { t1 += red[0][q * LPP + k][cl]; t2 += red[1][q * LPP + k][cl]; }
                const int gq = g0 + q;
                const double mu = mean[(long)gq * po.aff + c], rs = rstd[(long)gq * po.aff + c], gm = COEF ? gamma[c] : 0.f;
                const double dbe = t1, dga = rs * (t2 - mu * t1);
                if constexpr (COEF) {
                    const double c0 = gm * rs, m1 = dbe / count, m2 = dga / count;
                    const double c1 = -c0 * m2 * rs, c2 = -c0 * m1 - c1 * mu;
                    float* cf = coef + (long)gq * po.coef;
                    cf[c] = (float)c0; cf[C + c] = (float)c1; cf[2 * C + c] = (float)c2;
                }
                if (gq == 0 && !accumulate) { dg_run = (float)dga; db_run = (float)dbe; }
                else { dg_run = dg_run + (float)dga; db_run = db_run + (float)dbe; }
            }
        }
        __syncthreads();
    }
    if (rg == 0 && c < C && dgamma) { dgamma[c] = dg_run; dbeta[c] = db_run; }
}

}  // namespace
}  // namespace ustrun
