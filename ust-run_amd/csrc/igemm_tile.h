// igemm_tile.h -- what the three builds of the generic implicit-GEMM kernel share (igemm_f32_kernel in igemm.hip, igemm_bf16_kernel in
// igemm_bf16.hip, igemm_x3_kernel in x3.hip).  The builds differ in their middle only -- the LDS layout, how the weights arrive and
// which MFMA runs; the tile choice, the row table m -> (image, base pixel), the activation loader with its transform and the
// epilogue (scatter to one or two destinations, BatchNorm-statistics partials) are here, once.
#pragma once
#include "common.h"
#include "loader.h"

namespace ustrun {

// ---- tile choice (host) ------------------------------------------------------------------------------------------------------------
// Wave grid (WM x WN waves of 64 x 64 outputs) of the f32 and 16-bit builds: 128 x 128 for more than 64 output channels, 256 x 64
// below.  Pooled sources are built for the 128 x 128 tile only (narrow outputs behind a pooled source occur in tiny test nets).
struct IgemmTile { int wm, wn; bool pool; };
inline IgemmTile igemm_pick_tile(const IgemmArgs& a) {
    bool pool = false;
    for (int i = 0; i < a.nsrc; ++i) pool |= a.src[i].pool != 0;
    return (a.Cout > 64 || pool) ? IgemmTile{2, 2, pool} : IgemmTile{4, 1, false};
}

// ---- row table -----------------------------------------------------------------------------------------------------------------------
// row r of a tile = GEMM row m = mtile * BM + r = base pixel (n, by, bx); n = -1 past M.  (Extents < 65536: igemm_launch checks.)
struct RowInfo { int n; int yx; };
__device__ __forceinline__ int row_by(const RowInfo ri) { return ri.yx >> 16; }
__device__ __forceinline__ int row_bx(const RowInfo ri) { return ri.yx & 0xffff; }

// fills rowinfo[BM] (256 threads) and publishes it: ends with the block's barrier
template <int BM> __device__ __forceinline__ void fill_row_table(RowInfo* rowinfo, const IgemmArgs& a, int mtile, int tid) {
    for (int r = tid; r < BM; r += 256) {
        long m = (long)mtile * BM + r;
        RowInfo ri;
        if (m < a.M) {
            int hw = a.Hb * a.Wb;
            int n = (int)(m / hw);
            int rem = (int)(m - (long)n * hw);
            int by = rem / a.Wb;
            ri.n = n; ri.yx = (by << 16) | (rem - by * a.Wb);
        } else { ri.n = -1; ri.yx = 0; }
        rowinfo[r] = ri;
    }
    __syncthreads();
}

// ---- activation stage of the f32 and 16-bit builds -------------------------------------------------------------------------------
// What a thread holds of a stage between its fetch (under the previous stage's MFMAs) and its write to LDS: av = one 4-channel group
// of AR rows, NP stored pixels per logical pixel (4 under a 2x2 max-pool), asc / ash / a_relu = the group's BatchNorm constants,
// aok = the rows' in-bounds bits.
// Fetch for segment seg (tap offset d0 + (seg / segw, seg % segw) * dstep) the channels cg .. cg + 3 of rows a_r0 + RSTEP * i.
// vecA: 16-byte (ESZ = 4) or 8-byte (ESZ = 2) loads of raw values, transformed by activate(); otherwise the scalar path (first
// layer with C = 1/3, tiny test nets), where load_elem applies the transform here and activate() only copies.
template <int ESZ, bool POOL, int AR, int RSTEP>
__device__ __forceinline__ void load_a_stage(f32x4 (&av)[AR][POOL ? 4 : 1], f32x4& asc, f32x4& ash, int& a_relu, unsigned& aok,
                                             const IgemmArgs& a, const RowInfo* rowinfo, bool vecA, int seg, int cg, int a_r0) {
    const int dy = a.d0 + (seg / a.segw) * a.dstep, dx = a.d0 + (seg % a.segw) * a.dstep;
    aok = 0;
    asc = (f32x4){1.f, 1.f, 1.f, 1.f}; ash = (f32x4){0.f, 0.f, 0.f, 0.f}; a_relu = 0;
    if (vecA) {
        const bool second = (a.nsrc == 2 && cg >= a.src[0].C);
        const SrcDev S = pick_src(a.src[0], a.src[1], second);
        const int cl = cg - (second ? a.src[0].C : 0);
        const bool cok = cg < a.Cin;
        if (cok && S.scale) { asc = *(const f32x4*)(S.scale + cl); ash = *(const f32x4*)(S.shift + cl); }
        a_relu = S.relu;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const RowInfo ri = rowinfo[a_r0 + RSTEP * i];
            const int ly = row_by(ri) * a.s_in + dy - S.off_y;
            const int lx = row_bx(ri) * a.s_in + dx - S.off_x;
            const bool ok = cok && ri.n >= 0 && ly >= 0 && ly < S.LH && lx >= 0 && lx < S.LW;
            if (ok) {
                aok |= 1u << i;
                if constexpr (POOL) {
                    const long p = ri.n * S.sN + (long)(2 * ly) * S.sH + (long)(2 * lx) * S.sW + cl;
                    av[i][1] = ld4t<ESZ>(S.ptr, p + S.sW);
                    av[i][2] = ld4t<ESZ>(S.ptr, p + S.sH);
                    av[i][3] = ld4t<ESZ>(S.ptr, p + S.sH + S.sW);
                    av[i][0] = ld4t<ESZ>(S.ptr, p);      // last, as in the scalar arm below: hipcc joins the two arms' final stores, and
                                                         // were they to different elements, the joined store would index av at run time
                                                         // and put it in scratch
                } else {
                    av[i][0] = ld4t<ESZ>(S.ptr, ri.n * S.sN + (long)ly * S.sH + (long)lx * S.sW + cl);
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const RowInfo ri = rowinfo[a_r0 + RSTEP * i];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ri.n >= 0) {
                const int iy = row_by(ri) * a.s_in + dy, ix = row_bx(ri) * a.s_in + dx;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cg + j < a.Cin) v[j] = load_elem(a.src[0], a.src[1], a.nsrc, ri.n, iy, ix, cg + j);
            }
            av[i][0] = v;
        }
    }
}

// a row of the stage as it goes to LDS: affine, ReLU, the max over the pooling window, then zero outside the source (padding is
// applied after the activation)
template <int NP> __device__ __forceinline__ f32x4 activate(const f32x4 (&av)[NP], f32x4 asc, f32x4 ash, int a_relu, bool ok, bool vecA) {
    f32x4 v = av[0];
    if (vecA) {
        v = v * asc + ash;
        if (a_relu) v = relu4(v);
#pragma unroll
        for (int q = 1; q < NP; ++q) {
            f32x4 t = av[q] * asc + ash;
            if (a_relu) t = relu4(t);
            v = max4(v, t);
        }
        if (!ok) v = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    return v;
}

// ---- epilogue ----------------------------------------------------------------------------------------------------------------------
// The wave's 2 x 2 accumulators D[row = pixel][col = channel] (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) + bias ->
// output pixel base * s_out + (z >> 1, z & 1), channels [0, C0) to out0 and the rest to the window (o1y, o1x, H1, W1) of out1;
// with a.stat the column sums of the stored values and of their squares in a fixed order: the row chain of a lane, lane halves,
// then pairs of row waves through red[WM][2][BN] (LDS that is free after the main loop's final barrier).
// One statistics row per 128 pixels whatever the tile height, so that the row count does not depend on the tile configuration
// (igemm_mtiles, igemm_stat_rows_used, ustrun_conv_mtiles).
// OUT16: 16-bit storage -- the value is rounded before it is summed (statistics see the stored value), out0 is stored by a.out_esz
// (f32 outputs: the DeepLabV2 classifier maps), out1 is always 16-bit.
template <int WM, int WN, bool OUT16>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& a, const f32x16 (&acc)[2][2], const RowInfo* rowinfo, float* red,
                                               int mtile, int n0, int z, int tid) {
    constexpr int BN = WN * 64;
    const int wave = tid >> 6, wm = wave / WN, wn = wave % WN, l31 = tid & 31, lh = (tid >> 5) & 1;
    const int oyz = z >> 1, oxz = z & 1;
    const int C1 = a.Cout - a.C0;
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + j * 32 + l31;
        const bool cok = col < a.Cout;
        const float bias = (a.bias && cok) ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const RowInfo ri = rowinfo[row];
                if (ri.n >= 0 && cok) {
                    const bool o32 = !OUT16 || a.out_esz == 4;
                    const float v = o32 ? acc[i][j][r] + bias : rndt<2>(acc[i][j][r] + bias);
                    const int oy = row_by(ri) * a.s_out + oyz, ox = row_bx(ri) * a.s_out + oxz;
                    if (col < a.C0) {
                        const long oi = (((long)ri.n * a.Ho + oy) * a.Wo + ox) * a.C0 + col;
                        if (o32) st1t<4>(a.out0, oi, v); else st1t<2>(a.out0, oi, v);
                    } else {
                        const int y1 = oy - a.o1y, x1 = ox - a.o1x;
                        if (y1 >= 0 && y1 < a.H1 && x1 >= 0 && x1 < a.W1)
                            st1t<OUT16 ? 2 : 4>(a.out1, (((long)ri.n * a.H1 + y1) * a.W1 + x1) * C1 + (col - a.C0), v);
                    }
                    {   // the square is rounded before it is added (as every build of this epilogue has computed it): left to
                        // hipcc's contraction, whether this is one fused multiply-add depends on how the loop around it is scheduled
#pragma clang fp contract(off)
                        s1[j] += v; s2[j] += v * v;
                    }
                }
            }
        }
    }
    if (a.stat) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            s1[j] += __shfl_xor(s1[j], 32);
            s2[j] += __shfl_xor(s2[j], 32);
            if (lh == 0) {
                red[(wm * 2 + 0) * BN + wn * 64 + j * 32 + l31] = s1[j];
                red[(wm * 2 + 1) * BN + wn * 64 + j * 32 + l31] = s2[j];
            }
        }
        __syncthreads();
        constexpr int HALVES = WM / 2;
        const int stat_rows = (int)((a.M + 127) / 128);
        for (int t = tid; t < HALVES * 2 * BN; t += 256) {
            const int h = t / (2 * BN), q = (t / BN) % 2, c = t % BN;
            const float v = red[((2 * h) * 2 + q) * BN + c] + red[((2 * h + 1) * 2 + q) * BN + c];
            const int srow = mtile * HALVES + h;
            if (srow < stat_rows && n0 + c < a.Cout) a.stat[((long)srow * 2 + q) * a.Cout + n0 + c] = v;
        }
    }
}

}  // namespace ustrun
