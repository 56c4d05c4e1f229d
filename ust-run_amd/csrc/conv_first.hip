// conv_first.hip -- the network's first convolution (inc.conv0: C = 1..4 input channels, NCHW input,
// 64 outputs) and its weight gradient.  With K = 9*C <= 36 this layer is not a matrix-core problem:
// forward is HBM-bound on its 64-channel output (268 B/pixel written vs 12 B read), the weight gradient
// on reading dY once.
//
//  * forward: direct f32 stencil on the VALU.  8x16-pixel tile per block, lane = pixel, wave = group of
//    16 output channels; the 10x18xC input patch sits in LDS, the 27x16 weights of a wave are wave-uniform
//    (scalar loads, SGPR operands of v_fma).  Epilogue: NHWC f32 store + BatchNorm-statistics partials.
//  * weight gradient (bf16 MFMA): dW[(c,kh,kw)][co] = sum_p x[c][p+(kh,kw)-1] * dY[p][co] as a
//    [32 x pixels] x [pixels x 64] GEMM; the im2col rows are built in LDS from the NCHW patch (three
//    kw-shifted copies keep the 16-byte fragment reads aligned), dY tiles are read transposed.
//
// Shared with other files: conv_first_plan.h (the streaming kernels' strip plans, their item decodes and the one predicate for "the
// streaming weight gradient may run" -- ops.hip asks it too; pinned on the CPU by tests/host/conv_first_plan_check.hip), tn_gemm.h
// (the transposing fragment reads), x3_split.h (dtype USTRUN_F32X3's three-term split and its six-MFMA product).
#include "common.h"
#include "conv_first_plan.h"
#include "tn_gemm.h"
#include "x3_split.h"
#include <type_traits>

namespace ustrun {
namespace {

constexpr int FTH = 8, FTW = CF_WG_TW, FHW = FTW + 2, FHP = (FTH + 2) * FHW;   // 10 x 18 patch
constexpr int CMAX = 4;

// GEMM k index (= im2col row) -> (input channel, tap): k = 9 c + tap
__device__ __forceinline__ void k_decode(int k, int& c, int& tap) { c = k / 9; tap = k - c * 9; }

// the four waves' statistics partials red[wave][sum | sum of squares][channel] -> statistics row `row`, waves added in fixed order
__device__ __forceinline__ void sum_waves_store_stat(const float (&red)[4][2][64], float* __restrict__ stat, long row) {
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 128) {
        const int q = tid >> 6, c = tid & 63;
        stat[(row * 2 + q) * 64 + c] = red[0][q][c] + red[1][q][c] + red[2][q][c] + red[3][q][c];
    }
}

// x NCHW [N,C,H,W] (strides given), w = packed forward weights f32 [9][C][64], y NHWC [N,H,W,64], stat [tiles][2][64]
__global__ __launch_bounds__(256) void conv_first_fwd_kernel(const float* __restrict__ x, long sN, long sC, long sH, long sW,
                                                            int C, int H, int W, const float* __restrict__ w,
                                                            float* __restrict__ y, float* __restrict__ stat,
                                                            int tiles_x, int tiles_y) {
    __shared__ float patch[CMAX][FHP];
    __shared__ __attribute__((aligned(16))) float wl[CMAX * 9][64];   // weights as [c*9+t][co]
    __shared__ float red[4][2][16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 16 output channels per wave
    const int img = blockIdx.x / (tiles_y * tiles_x);
    const int rem = blockIdx.x - img * tiles_y * tiles_x;
    const int y0 = (rem / tiles_x) * FTH, x0 = (rem % tiles_x) * FTW;
    for (int t = tid; t < C * FHP; t += 256) {
        const int c = t / FHP, hp = t - c * FHP;
        const int iy = y0 + hp / FHW - 1, ix = x0 + hp % FHW - 1;
        patch[c][hp] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[img * sN + c * sC + iy * sH + ix * sW] : 0.f;
    }
    for (int t = tid; t < C * 9 * 64; t += 256) {                    // packed forward weights -> [c*9+tap][co]
        const int co = t & 63, k = t >> 6;
        int c, tap;
        k_decode(k, c, tap);
        wl[k][co] = w[((long)tap * C + c) * 64 + co];
    }
    __syncthreads();
    float s1[16], s2[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
#pragma unroll
    for (int g = 0; g < 2; ++g) {                                   // two 4x16 pixel groups per block
        const int py = g * 4 + (lane >> 4), px = lane & 15;
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float v = patch[c][(py + t / 3) * FHW + px + t % 3];
                const float* wk = &wl[c * 9 + t][wave * 16];          // wave-uniform address: LDS broadcast
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 w4 = *(const f32x4*)(wk + 4 * q);
                    acc[4 * q] = fmaf(v, w4[0], acc[4 * q]); acc[4 * q + 1] = fmaf(v, w4[1], acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(v, w4[2], acc[4 * q + 2]); acc[4 * q + 3] = fmaf(v, w4[3], acc[4 * q + 3]);
                }
            }
        const int oy = y0 + py, ox = x0 + px;
        if (oy < H && ox < W) {
            const long o = (((long)img * H + oy) * W + ox) * 64 + wave * 16;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(y + o + 4 * q) = (f32x4){acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
#pragma unroll
            for (int j = 0; j < 16; ++j) { s1[j] += acc[j]; s2[j] += acc[j] * acc[j]; }
        }
    }
    if (stat) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float a = s1[j], b = s2[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
            if (lane == 0) { red[wave][0][j] = a; red[wave][1][j] = b; }
        }
        __syncthreads();
        if (tid < 128) {
            const int q = tid >> 6, c = tid & 63;
            stat[((long)blockIdx.x * 2 + q) * 64 + c] = red[c >> 4][q][c & 15];
        }
    }
}

// ---- forward on the bf16 matrix cores (dtype = bf16) ---------------------------------------------
// The f32 stencil above is VALU-bound (27*64 FMAs per pixel: 134 us at N=16, 256^2) while the layer only has to
// write 134 MB.  As an im2col GEMM [pixels x 9C] x [9C x 64] with K padded to 16*KS it is a handful of MFMAs:
// 8x32-pixel tile per block, the (10 x 34 x C) f32 patch in LDS, every lane gathers the 8 K-values of its pixel
// with ds_read_b32 at per-lane constant offsets (k -> (c, tap)) and rounds them to bf16; the weight fragments are
// block constants kept in registers.  Epilogue as in conv_halo_bf16.hip: per-wave LDS transpose, 16-byte stores,
// BatchNorm-statistics partials of the stored values (one row per block).
constexpr int MTH = CF_FWD_TH, MTW = CF_FWD_TW, MHW = MTW + 2, MHP = (MTH + 2) * MHW;   // 10 x 34 patch

template <int KS>
__global__ __launch_bounds__(256, 4) void conv_first_fwd_mfma_kernel(const float* __restrict__ x, long sN, long sC, long sH, long sW,
                                                                    int C, int H, int W, const elt_t* __restrict__ w,
                                                                    elt_t* __restrict__ y, float* __restrict__ stat,
                                                                    int tiles_x, int tiles_y) {
    constexpr int EPITCH = 144;
    __shared__ float patch[CMAX * MHP + 4];                 // [c][10][34]; the last word stays zero (K padding)
    __shared__ __attribute__((aligned(16))) elt_t Bw[KS * 2][64][8];
    __shared__ __attribute__((aligned(16))) char eps[4 * 32 * EPITCH];
    __shared__ float red[4][2][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int img = blockIdx.x / (tiles_y * tiles_x);
    const int rem = blockIdx.x - img * tiles_y * tiles_x;
    const int y0 = (rem / tiles_x) * MTH, x0 = (rem % tiles_x) * MTW;
    const int K = 9 * C;
    for (int t = tid; t < C * MHP; t += 256) {
        const int c = t / MHP, hp = t - c * MHP;
        const int iy = y0 + hp / MHW - 1, ix = x0 + hp % MHW - 1;
        patch[t] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[img * sN + c * sC + iy * sH + ix * sW] : 0.f;
    }
    if (tid < 4) patch[CMAX * MHP + tid] = 0.f;
    for (int t = tid; t < KS * 2 * 64 * 8; t += 256) {       // k = c*9 + tap; packed forward weights are [tap][1][64][8 (c)]
        const int j = t & 7, co = (t >> 3) & 63, k8 = t >> 9, k = k8 * 8 + j;
        int c, tap;
        k_decode(k, c, tap);
        Bw[k8][co][j] = k < K ? w[((long)tap * 64 + co) * 8 + c] : (elt_t)0.f;
    }
    // this lane's K entries: k = 16 ks + 8 lh + j -> patch offset relative to the pixel's (0,0) tap
    int koff[KS][8];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * ks + 8 * lh + j;
            int c, tap;
            k_decode(k, c, tap);
            koff[ks][j] = k < K ? c * MHP + (tap / 3) * MHW + tap % 3 : -1;
        }
    __syncthreads();
    bf16x8 bfr[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        bfr[ks][0] = *(const bf16x8*)&Bw[2 * ks + lh][l31][0];
        bfr[ks][1] = *(const bf16x8*)&Bw[2 * ks + lh][32 + l31][0];
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {                            // wave owns tile rows 2*wave + i, 32 pixels each
        const int base = (2 * wave + i) * MHW + l31;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 af;
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = (elt_t)patch[koff[ks][j] >= 0 ? base + koff[ks][j] : CMAX * MHP];
            acc[i][0] = USTRUN_MFMA_32x32x16(af, bfr[ks][0], acc[i][0], 0, 0, 0);
            acc[i][1] = USTRUN_MFMA_32x32x16(af, bfr[ks][1], acc[i][1], 0, 0, 0);
        }
    }
    // epilogue
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
    char* ep = eps + wave * (32 * EPITCH);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int oy = y0 + 2 * wave + i;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const elt_t hv = (elt_t)acc[i][n][r];
                *(elt_t*)(ep + row * EPITCH + (n * 32 + l31) * 2) = hv;
                if (oy < H && x0 + row < W) {
                    const float v = (float)hv;                 // statistics see the stored value
                    s1[n] += v; s2[n] += v * v;
                }
            }
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int idx = lane + 64 * t, row = idx >> 3, ch = idx & 7;
            const bf16x8 v8 = *(const bf16x8*)(ep + row * EPITCH + ch * 16);
            const int ox = x0 + row;
            if (oy < H && ox < W) *(bf16x8*)(y + (((long)img * H + oy) * W + ox) * 64 + ch * 8) = v8;
        }
        wave_lds_sync();
    }
    if (stat) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            s1[n] += __shfl_xor(s1[n], 32);
            s2[n] += __shfl_xor(s2[n], 32);
            if (lh == 0) { red[wave][0][n * 32 + l31] = s1[n]; red[wave][1][n * 32 + l31] = s2[n]; }
        }
        sum_waves_store_stat(red, stat, blockIdx.x);
    }
}

// ---- weight gradient -----------------------------------------------------------------------
// block: a range of 8x16 tiles; wave w owns tile rows {2w, 2w+1}: D[32 im2col rows][64 co] per wave,
// waves summed through LDS at the end, one slab per block: slab[(c*9 + t)][co] (rows >= 9C unused)
constexpr int WRB = 192;     // dY LDS row pitch (64 bf16 + pad: conflict-free transposed reads)

// a lane's byte offset into a [16 px][WRB] dY tile for tr_frag_rows: pixel row 8 lh + q, columns 16 ((l >> 4) & 1) + 4 (l & 3) ..
__device__ __forceinline__ int dy_lane_base(int lane) {
    const int lh = lane >> 5, lrow = 8 * lh + ((lane & 15) >> 2), lcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    return lrow * WRB + lcol * 2;
}

// Block epilogue of both weight-gradient kernels: sum the four waves' accumulators (fixed order, 0 + 1 + 2 + 3) through LDS and write
// the block's slab.  accs lives in the dY tiles' memory, hence the barrier in front: every wave is done reading its last tile.
__device__ __forceinline__ void sum_waves_store_slab(const f32x16 (&acc)[2], float (*accs)[32][64], float* __restrict__ partials) {
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) accs[wave][(r & 3) + 8 * (r >> 2) + 4 * lh][j * 32 + l31] = acc[j][r];
    __syncthreads();
    float* slab = partials + (long)blockIdx.x * 32 * 64;
    for (int e = tid; e < 32 * 64; e += 256) {
        const int i = e >> 6, co = e & 63;
        slab[e] = accs[0][i][co] + accs[1][i][co] + accs[2][i][co] + accs[3][i][co];
    }
}

// the tile kernel of rounds 1-4 (16-bit dY): the fallback for layouts outside the streaming kernel's range, and ustrun_debug_flags bit 28
__global__ __launch_bounds__(256) void conv_first_wgrad_kernel(const float* __restrict__ x, long sN, long sC, long sH, long sW,
                                                              int C, int H, int W, const elt_t* __restrict__ dy,
                                                              float* __restrict__ partials, int tiles_x, int tiles_y,
                                                              int ttotal, int tiles_per) {
    // im2col source: xs[c][kw][hy][16] bf16 = patch shifted by kw so that 8 consecutive pixels are 16-B aligned
    __shared__ __attribute__((aligned(16))) elt_t xs[CMAX][3][FTH + 2][FTW];
    // (the end-of-block sum of the four waves' accumulators reuses the dY tile's memory: 36 KB per block instead of 60 -- all
    // 1024 blocks, four per CU, are resident at once; with 60 KB two per CU were, and the kernel ran its grid in two rounds)
    constexpr int DYSB = FTH * FTW * WRB > 4 * 32 * 64 * 4 ? FTH * FTW * WRB : 4 * 32 * 64 * 4;
    __shared__ __attribute__((aligned(16))) char dys[DYSB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    // this lane's im2col row i = l31 -> (c, kh, kw); rows >= 9C are zero
    int ic, it;
    k_decode(l31, ic, it);
    const int ikh = it / 3, ikw = it % 3;
    const bool ivalid = l31 < 9 * C;
    const char* lbase = dys + dy_lane_base(lane);

    const int tbeg = blockIdx.x * tiles_per, tend = min(ttotal, tbeg + tiles_per);
    // Register-staged software pipeline: the next tile's dY (16 B per item) and x elements are loaded while the current
    // tile's MFMAs run (the synchronous load -> barrier -> compute loop spent 16 us per 16 KB tile).  The decomposition
    // of this thread's x elements into (channel, kw, patch row, pixel) does not depend on the tile.
    constexpr int XIT = (CMAX * 3 * (FTH + 2) * FTW + 255) / 256;
    constexpr int DIT = FTH * FTW * 8 / 256;                         // 16-byte items: 8 channels
    int xdec[XIT];
#pragma unroll
    for (int i = 0; i < XIT; ++i) {
        const int e = tid + 256 * i;
        const int px = e % FTW, hy = (e / FTW) % (FTH + 2), kw = (e / (FTW * (FTH + 2))) % 3, c = e / (FTW * (FTH + 2) * 3);
        xdec[i] = e < C * 3 * (FTH + 2) * FTW ? (c << 16) | (kw << 12) | (hy << 6) | px : -1;
    }
    float xr[XIT];
    f32x4 dr[DIT];
    auto prefetch = [&](int t) {
        const int img = t / (tiles_y * tiles_x);
        const int rem = t - img * tiles_y * tiles_x;
        const int y0 = (rem / tiles_x) * FTH, x0 = (rem % tiles_x) * FTW;
#pragma unroll
        for (int i = 0; i < XIT; ++i) {
            const int d = xdec[i];
            const int c = d >> 16, kw = (d >> 12) & 3, hy = (d >> 6) & 63, px = d & 63;
            const int iy = y0 + hy - 1, ix = x0 + px + kw - 1;
            xr[i] = (d >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[img * sN + c * sC + iy * sH + ix * sW] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < DIT; ++i) {
            const int e = tid + 256 * i;
            const int p = e >> 3, g = e & 7;
            const int oy = y0 + (p >> 4), ox = x0 + (p & 15);
            dr[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (oy < H && ox < W) dr[i] = *(const f32x4*)(dy + (((long)img * H + oy) * W + ox) * 64 + 8 * g);
        }
    };
    if (tbeg < tend) prefetch(tbeg);
    for (int t = tbeg; t < tend; ++t) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XIT; ++i) {
            const int d = xdec[i];
            if (d >= 0) xs[d >> 16][(d >> 12) & 3][(d >> 6) & 63][d & 63] = (elt_t)xr[i];
        }
#pragma unroll
        for (int i = 0; i < DIT; ++i) {
            const int e = tid + 256 * i;
            *(f32x4*)(dys + (e >> 3) * WRB + (e & 7) * 16) = dr[i];              // 8 elements, as stored
        }
        if (t + 1 < tend) prefetch(t + 1);
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int r = wave * 2 + rr;                              // tile row = 16 pixels = one MFMA k-step
            bf16x8 a;
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = (elt_t)0.f;
            if (ivalid) a = *(const bf16x8*)&xs[ic][ikw][r + ikh][8 * lh];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = USTRUN_MFMA_32x32x16(a, tr_frag_rows<WRB>(lbase + j * 64, r * FTW), acc[j], 0, 0, 0);
        }
    }
    sum_waves_store_slab(acc, (float (*)[32][64])dys, partials);
}

// ---- weight gradient, streaming form (round 5) -----------------------------------------------------------------------------
// The layer is a 537 MB read of dY (N = 64) beside 17 GFLOP: the tile kernel above moved it at 2.8 TB/s -- 4 MFMAs per wave between
// two block barriers per 16 KB tile, one tile of prefetch.  Here nothing is shared between waves: a wave owns a 16-pixel-wide strip
// of `seg_rows` rows of one image and walks it a row a step; a step's dY row piece (16 px x 64 ch = 2 KB, contiguous) and the eight
// x values of the lane's im2col row (c, kh, kw) -- straight from the NCHW image, which stays in L2 -- are fetched into REGISTERS
// four steps ahead (the compiler counts those waits itself), the dY piece passes through a wave-private LDS slot for the
// transposing fragment reads, two MFMAs, next step.  No barrier until the block's four accumulator sets are summed at the end.
//
// One walk, two builds.  `Op` supplies what differs: the dY element, how many 16-byte pieces of a row piece a lane fetches, how a
// piece lands in the slot, how the x values become the A fragment, and the product.  The pieces' geometry follows from the bytes
// per pixel: the lane fetches piece 64 i + lane of the row piece = pixel PXS i + lane / PPP, 16-byte channel group lane % PPP.
template <int PXB_, int PLANES> struct WgPieces {
    static constexpr int PXB = PXB_;                     // bytes of dY per pixel
    static constexpr int PPP = PXB / 16;                 // pieces per pixel
    static constexpr int PXS = 64 / PPP;                 // pixels a wave covers with one piece per lane
    static constexpr int NP = FTW / PXS;                 // pieces per lane per row
    static constexpr int SLOT = PLANES * FTW * WRB;      // LDS bytes of one row piece: PLANES planes of [16 px][WRB] 16-bit values
    static constexpr int LDS = 4 * 2 * SLOT > 4 * 32 * 64 * 4 ? 4 * 2 * SLOT : 4 * 32 * 64 * 4;   // 4 waves x 2 slots, >= the final sum's 32 KB
    static __device__ __forceinline__ int px(int i, int lane) { return PXS * i + lane / PPP; }
    static __device__ __forceinline__ int mem_off(int i, int lane) { return px(i, lane) * PXB + (lane % PPP) * 16; }           // in the row piece
    static __device__ __forceinline__ int lds_off(int i, int lane) { return px(i, lane) * WRB + (lane % PPP) * (2048 / PXB); }  // in a plane
};

// d & m, one dword at a time (written as one vector operation the 16-bit build takes 152 VGPRs instead of 116: a block per CU less)
__device__ __forceinline__ u32x4 and4(u32x4 d, unsigned m) {
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] &= m;
    return d;
}

struct WgOp16 : WgPieces<128, 1> {                       // 16-bit dY (2 KB per step), used as stored: one MFMA per column half
    typedef elt_t dy_t;
    typedef bf16x8 afrag;
    static constexpr bool BN = false;
    static constexpr const char* NAME = "conv_first_wgrad_stream";
    static __device__ __forceinline__ void stage(char* sl, int lane, const u32x4 (&d)[NP], const unsigned (&m)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) *(u32x4*)(sl + lds_off(i, lane)) = and4(d[i], m[i]);
    }
    static __device__ __forceinline__ afrag a_frag(const float (&v)[8]) {
        afrag a;
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = (elt_t)v[q];
        return a;
    }
    static __device__ __forceinline__ void multiply(const afrag& a, const char* lbase, f32x16 (&acc)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = USTRUN_MFMA_32x32x16(a, tr_frag_rows<WRB>(lbase + j * 64, 0), acc[j], 0, 0, 0);
    }
};

// The same with dY formed on load: the layer's BatchNorm-backward apply pass, dy = k0 (a > 0 ? da : 0) + k1 y + k2, runs on each
// 16-byte piece (8 channels of a pixel: the lane's channel group lane % 8 is the same for all its pieces, its 40 constants live in
// registers) of da and y as they come out of the prefetch registers -- bn_bwd_apply8, the statement of the apply kernel, rounded to
// the storage type like its store -- and the MFMA gets the registers the stored dy would have filled.  4 KB per step instead of 2,
// no apply pass (read da, y; write dy) in front and no dy to read back.
struct WgOp16Bn : WgOp16 {
    static constexpr bool BN = true;
    static constexpr const char* NAME = "conv_first_wgrad_stream_bn";
};

struct WgOpX3 : WgPieces<256, 3> {                       // dtype USTRUN_F32X3: f32 dY (4 KB per step), both operands split into three
    typedef float dy_t;                                  // bf16 terms at use (x3.hip's arithmetic: six MFMAs per product, f32-level
    struct afrag { b16x8 p[3]; };                        // result), three LDS planes per slot
    static constexpr bool BN = false;
    static constexpr const char* NAME = "conv_first_wgrad_x3";
    static __device__ __forceinline__ void stage(char* sl, int lane, const u32x4 (&d)[NP], const unsigned (&m)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) store_planes(split3(__builtin_bit_cast(f32x4, and4(d[i], m[i]))), sl + lds_off(i, lane), FTW * WRB);
    }
    static __device__ __forceinline__ afrag a_frag(const float (&v)[8]) {
        u32x2 lo[3], hi[3];
        split4((f32x4){v[0], v[1], v[2], v[3]}, lo[0], lo[1], lo[2]);
        split4((f32x4){v[4], v[5], v[6], v[7]}, hi[0], hi[1], hi[2]);
        afrag a;
#pragma unroll
        for (int p = 0; p < 3; ++p) a.p[p] = __builtin_bit_cast(b16x8, (u32x4){lo[p][0], lo[p][1], hi[p][0], hi[p][1]});
        return a;
    }
    static __device__ __forceinline__ void multiply(const afrag& a, const char* lbase, f32x16 (&acc)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            b16x8 b[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) b[p] = tr_frag_rows<WRB, __bf16>(lbase + p * FTW * WRB + j * 64, 0);
            acc[j] = mfma6(a.p, b, acc[j]);
        }
    }
};

// Op::BN: dy holds da; y and the BatchNorm-backward constants of the pass an image belongs to (image / gN) come with it
struct CfWgradBn { const void* y; const float* scale; const float* shift; const float* coef; int gN; int aff_stride; int coef_stride; };

template <typename Op, int D>
__global__ __launch_bounds__(256) void conv_first_wgrad_stream_kernel(const float* __restrict__ x, int sN, int sC, int sH, int C,
                                                                      int H, int W, int xbytes, const typename Op::dy_t* __restrict__ dy,
                                                                      int dybytes, float* __restrict__ partials, int strips, int segs,
                                                                      int seg_rows, int items, const CfWgradBn bn) {
    constexpr int NP = Op::NP;
    extern __shared__ __attribute__((aligned(16))) char dys[];        // Op::LDS bytes: 4 waves x 2 slots, then the final sum
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const int item = blockIdx.x * 4 + wave;
    if (item < items) {
        const CfWgradItem w = conv_first_wgrad_item(strips, segs, seg_rows, H, item);
        const int img = w.img, x0 = w.x0, r0 = w.r0, r1 = w.r1;
        // this lane's im2col row i = l31 -> (c, kh, kw); rows >= 9C are zero
        int ic, it;
        k_decode(l31, ic, it);
        const int ikh = it / 3, ikw = it % 3;
        const bool ivalid = l31 < 9 * C;
        // Both tensors are read through ONE buffer resource each, every load issued unconditionally: an offset outside the tensor
        // (one float in front of the first row, a few behind the last) fails the range check and returns zeros; what must not
        // count -- image rows above / below, columns left / right of the image, im2col rows past 9 C, rows past the segment --
        // is masked when the values are USED, four steps later: a select around a load would put its wait right behind the load.
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, xbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, dybytes, 0x00020000);
        const int col0 = x0 + 8 * lh + ikw - 1;                       // first of the lane's eight pixels' x columns
        // (the one lane column that starts a float in FRONT of its row -- x0 = 0, kw = 0 -- would start the tensor's very first row at
        // offset -4: the whole 16-byte load fails the range check, not just its first word.  Those lanes fetch one column to the
        // right and shift the values back when they use them.)
        const bool shl = col0 < 0;
        const int xoff0 = (img * sN + (ivalid ? ic : 0) * sC + col0 + (shl ? 1 : 0)) * 4;
        unsigned cm[8];                                               // per column: all ones where it lies in the image
#pragma unroll
        for (int q = 0; q < 8; ++q) cm[q] = (ivalid && (unsigned)(col0 + q) < (unsigned)W) ? 0xffffffffu : 0u;
        unsigned dm[NP];                                              // per dY piece: all ones where its pixel lies in the image
#pragma unroll
        for (int i = 0; i < NP; ++i) dm[i] = x0 + Op::px(i, lane) < W ? 0xffffffffu : 0u;
        const int doff0 = (img * H * W + x0) * Op::PXB + Op::mem_off(0, lane);
        char* slot = dys + wave * (2 * Op::SLOT);
        const int lbase = dy_lane_base(lane);
        u32x4 xr[D][2], dr[D][NP];
        unsigned rm[D];                                               // per slot: all ones where the lane's x row lies in the image
        // Op::BN: y's pieces ride with da's through the same offsets; the lane's channel group and the item's pass are fixed
        constexpr int NY = Op::BN ? NP : 1;
        u32x4 yr[D][NY];
        __amdgpu_buffer_rsrc_t ry = rd;
        F8 bsc = {}, bsh = {}, bk0 = {}, bk1 = {}, bk2 = {};
        if constexpr (Op::BN) {
            ry = __builtin_amdgcn_make_buffer_rsrc((void*)bn.y, 0, dybytes, 0x00020000);
            const int ps = img / bn.gN, c8 = 8 * (lane % Op::PPP);
            const float* cf = bn.coef + (long)ps * bn.coef_stride + c8;
            bsc = ld8f(bn.scale + (long)ps * bn.aff_stride + c8); bsh = ld8f(bn.shift + (long)ps * bn.aff_stride + c8);
            bk0 = ld8f(cf); bk1 = ld8f(cf + 64); bk2 = ld8f(cf + 128);
        }
        auto prefetch = [&](int u, int y) {
            const int yy = y + ikh - 1;
            rm[u] = (y < r1 && (unsigned)yy < (unsigned)H) ? 0xffffffffu : 0u;
            const int xo = xoff0 + yy * sH * 4;
            xr[u][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, xo, 0, 0));
            xr[u][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, xo + 16, 0, 0));
            const int dofs = doff0 + min(y, r1 - 1) * W * Op::PXB;
#pragma unroll
            for (int i = 0; i < NP; ++i)
                dr[u][i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rd, dofs + i * Op::PXS * Op::PXB, 0, 0));
            if constexpr (Op::BN) {
#pragma unroll
                for (int i = 0; i < NP; ++i)
                    yr[u][i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ry, dofs + i * Op::PXS * Op::PXB, 0, 0));
            }
        };
        auto consume = [&](int u, int par, bool live) {
            char* sl = slot + par * Op::SLOT;
            const unsigned lm = live ? 0xffffffffu : 0u;              // (wave-uniform: rows past the segment add nothing)
            unsigned m[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) m[i] = dm[i] & lm;
            if constexpr (Op::BN) {     // (pieces outside the image or the segment become some k2 here and zero under the mask in stage)
#pragma unroll
                for (int i = 0; i < NP; ++i)
                    dr[u][i] = __builtin_bit_cast(u32x4, bn_bwd_apply8(__builtin_bit_cast(bf16x8, yr[u][i]), __builtin_bit_cast(bf16x8, dr[u][i]),
                                                                       bsc, bsh, bk0, bk1, bk2));
            }
            Op::stage(sl, lane, dr[u], m);
            unsigned v[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[q] = xr[u][0][q]; v[4 + q] = xr[u][1][q]; }
            float f[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned t = shl ? (q ? v[q - 1] : 0u) : v[q];
                f[q] = __builtin_bit_cast(float, t & cm[q] & rm[u]);
            }
            Op::multiply(Op::a_frag(f), sl + lbase, acc);
        };
#pragma unroll
        for (int u = 0; u < D; ++u) prefetch(u, r0 + u);
        for (int y = r0; y < r1; y += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                consume(u, u & 1, y + u < r1);
                prefetch(u, y + u + D);
            }
        }
    }
    sum_waves_store_slab(acc, (float (*)[32][64])dys, partials);
}

// dw[co][c][t] (+)= sum_k partials[k][c*9+t][co].  Block = 8 outputs (consecutive co of one im2col row: 32 contiguous bytes per
// slab) x 128 slab lanes; a lane's slabs k = lane, lane + 128, .. are ALL loaded before the first add (up to eight in flight: the
// 1024-slab table is one memory round trip, where 32 lanes x four in flight made it eight dependent ones -- 35 us for 8 MB), summed
// in ascending k, then the lanes in ascending order: a fixed order, f64.
__global__ __launch_bounds__(1024) void conv_first_wgrad_reduce_kernel(const float* __restrict__ partials, int nslab, int C,
                                                                     float* __restrict__ dw, int accumulate) {
    __shared__ double red[128][8];
    const int ol = threadIdx.x & 7, sl = threadIdx.x >> 3;
    const int e = blockIdx.x * 8 + ol;                   // (im2col row i, co) in i-major order
    const int i = e >> 6, co = e & 63;
    double v = 0.0;
    if (i < 9 * C) {
        const float* p0 = partials + (long)i * 64 + co;
        for (int k0 = sl; k0 < nslab; k0 += 1024) {
            float a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int k = k0 + 128 * u; a[u] = p0[(long)(k < nslab ? k : k0) * 2048]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) v += (k0 + 128 * u < nslab) ? (double)a[u] : 0.0;
        }
    }
    red[sl][ol] = v;
    __syncthreads();
    if (sl == 0 && i < 9 * C) {
        for (int k = 1; k < 128; ++k) v += red[k][ol];
        const int o = co * (C * 9) + i;
        dw[o] = accumulate ? dw[o] + (float)v : (float)v;
    }
}

// ---- forward, streaming form (round 4) -------------------------------------------------------------------------------------
// The layer writes 128 B per pixel and reads 12: it is a store stream with a little arithmetic in front.  The tile-per-block
// kernel above pays its whole setup (weight fragments through LDS, k -> patch offsets with divisions, a patch fill whose loads
// nothing overlaps) for 256 pixels and then stores through 2-byte LDS writes: 3.0-3.2 TB/s of output where the BatchNorm
// passes, which move the same kind of bytes, reach 5.4.  Here a block owns a 32-pixel-wide strip of `seg_rows` rows of one
// image and walks it 8 rows per step: weight fragments (the A operand: rows = output channels) and the k -> patch index
// tables are built once per block and live in registers; the next step's 10 x 34 x C input patch is fetched into registers
// under the current step's work and lands in the other LDS buffer; the product is D[channel][pixel], so four consecutive
// channels of a pixel sit in four consecutive accumulator registers: 2 cvt_pk + ONE ds_write_b64 per group into a per-wave
// scratch, read back as 16-byte pieces (8 channels of one pixel per lane) that go out as whole 128-byte lines; the BatchNorm
// statistics are taken from those pieces (8 channels per lane, 16 accumulators) and leave the block ONCE, as one row per block.
constexpr int SPITCH = 144;          // scratch row: 128 B of channels + 16 B pad (16-byte aligned rows)

template <int C, bool STAT>
__global__ __launch_bounds__(256, 3) void conv_first_fwd_stream_kernel(const float* __restrict__ x, long sN, int sC, int sH, int sW,
                                                                      int H, int W, const elt_t* __restrict__ w,
                                                                      elt_t* __restrict__ y, float* __restrict__ stat,
                                                                      CfFwdPlan plan, int img_bytes) {
    constexpr int KS = (9 * C + 15) / 16;
    constexpr int PROWS = MTH + 2;                          // patch rows of a step
    // one patch buffer (floats): [c][10][34], then a ZERO AREA that padded k entries read: a lane's k -> patch index table is
    // built for its first row of a step and the second row is the same table + one patch row (an immediate offset), so a
    // padded entry reads ZIDX and ZIDX + MHW
    constexpr int ZIDX = CMAX * MHP;
    constexpr int PSZ = ZIDX + MHW + 6;
    __shared__ float patch[2 * PSZ];
    __shared__ __attribute__((aligned(16))) char scr[4 * 32 * SPITCH];
    __shared__ float red[4][2][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: the stores' row offset is a scalar operand
    const int l31 = lane & 31, lh = lane >> 5;
    const int item = blockIdx.x;
    const CfFwdItem it = conv_first_fwd_item(plan, H, item);
    const int img = it.img, x0 = it.x0, r0 = it.r0, r1 = it.r1, nsteps = it.nsteps;
    constexpr int K = 9 * C;
    // every access to the image and to the output goes through a buffer resource of ONE image: an offset with bit 31 set fails
    // the range check (loads return 0, stores are dropped), so padding and ragged edges need no branch around a memory
    // instruction (hipcc turns a select around a load into a branch with its own wait: the prefetch would serialise)
    constexpr int OOB = (int)0x80000000;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + img * sN), 0, img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(y + (long)img * H * W * 64), 0, H * W * 128, 0x00020000);
    // weight fragments, A operand of D[co][px] = W[co][k] P[k][px]: lane (row = co, half lh) holds k = 16 ks + 8 lh + j;
    // packed forward weights are [tap][1][64][8 (c)]
    bf16x8 wf[KS][2];
    int kidx[KS][8];                                       // BYTE offset into a patch buffer of k's entry for (row 2 wave, pixel l31)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * ks + 8 * lh + j;
            int c, tap;
            k_decode(k, c, tap);
            const bool kv = k < K;
            wf[ks][0][j] = kv ? w[((long)tap * 64 + l31) * 8 + c] : (elt_t)0.f;
            wf[ks][1][j] = kv ? w[((long)tap * 64 + 32 + l31) * 8 + c] : (elt_t)0.f;
            kidx[ks][j] = (kv ? c * MHP + (tap / 3 + 2 * wave) * MHW + tap % 3 + l31 : ZIDX) * 4;
        }
    // patch fetch: thread t < 34 C owns patch column (c, px) = (t / 34, t % 34) and fetches its 10 rows -- the row part of the
    // address and its validity are wave-uniform, the column part is a per-thread constant
    const bool loader = tid < C * MHW;
    const int lc = tid / MHW, lpx = tid - lc * MHW, lix = x0 - 1 + lpx;
    const int coloff = (loader && lix >= 0 && lix < W) ? (lc * sC + lix * sW) * 4 : OOB;
    const int lds_col = (lc * MHP + lpx) * 4;
    float pre[PROWS];
    auto load = [&](int s) {
        const int yb = r0 + MTH * s - 1;
#pragma unroll
        for (int i = 0; i < PROWS; ++i) {
            const int iy = yb + i;                          // (uniform)
            const int voff = (iy >= 0 && iy < H) ? coloff : OOB;
            pre[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, voff, iy * sH * 4, 0));
        }
    };
    for (int t = tid; t < MHW + 6; t += 256) { patch[ZIDX + t] = 0.f; patch[PSZ + ZIDX + t] = 0.f; }
    float s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    char* ep = scr + wave * (32 * SPITCH);
    if (loader) load(0);
    auto step = [&](int s, auto buf_c) {
        constexpr int buf = decltype(buf_c)::value;
        const char* P = (const char*)(patch + buf * PSZ);
        if (loader) {
#pragma unroll
            for (int i = 0; i < PROWS; ++i) *(float*)((char*)(patch + buf * PSZ) + lds_col + i * MHW * 4) = pre[i];
        }
        __syncthreads();                                  // (also: every wave is done with the buffer the NEXT step fills)
        if (loader && s + 1 < nsteps) load(s + 1);        // in flight under this step's work
        const int yb = r0 + MTH * s;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oy = yb + 2 * wave + i;
            f32x16 acc[2];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (elt_t) * (const float*)(P + kidx[ks][j] + i * MHW * 4);
                acc[0] = USTRUN_MFMA_32x32x16(wf[ks][0], pf, acc[0], 0, 0, 0);
                acc[1] = USTRUN_MFMA_32x32x16(wf[ks][1], pf, acc[1], 0, 0, 0);
            }
            // D row (channel) = (r & 3) + 8 (r >> 2) + 4 lh, column (pixel) = l31: registers 4g .. 4g + 3 = channels 8g + 4lh + 0..3
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 h4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) h4[q] = (elt_t)acc[n][4 * g + q];
                    *(bf16x4*)(ep + l31 * SPITCH + (n * 32 + 8 * g + 4 * lh) * 2) = h4;
                }
            wave_lds_sync();
            const bool rowok = oy < r1;                    // (uniform)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int idx = lane + 64 * t, pr = idx >> 3, ch = idx & 7;        // ch == lane & 7 for every t
                const bf16x8 v8 = *(const bf16x8*)(ep + pr * SPITCH + ch * 16);
                const int ox = x0 + pr;
                const bool ok = rowok && ox < W;
                // (the row offset rides in the VECTOR offset, soffset stays 0: with an SGPR soffset hipcc's hazard recognizer inserts no
                // wait state between a 128-bit buffer store and a VALU write of its data registers -- an SI-era rule -- and on gfx950,
                // with the store pipe saturated, the store then ships the overwritten dword for the last lanes of each 16:
                // 6e-6 of the outputs in the no-statistics build, none in the build whose statistics code sits in between)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v8), ry, ok ? ((oy * W + ox) * 64 + ch * 8) * 2 : OOB, 0, 0);
                if constexpr (STAT) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float v = ok ? (float)v8[j] : 0.f;             // statistics see the stored value
                        s1[j] += v; s2[j] += v * v;
                    }
                }
            }
            wave_lds_sync();
        }
    };
    for (int s = 0; s < nsteps; s += 2) {
        step(s, std::integral_constant<int, 0>{});
        if (s + 1 < nsteps) step(s + 1, std::integral_constant<int, 1>{});
    }
    if constexpr (STAT) {                                  // lanes with equal lane & 7 hold the same 8 channels
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) { s1[j] += __shfl_xor(s1[j], o); s2[j] += __shfl_xor(s2[j], o); }
            if (lane < 8) { red[wave][0][lane * 8 + j] = s1[j]; red[wave][1][lane * 8 + j] = s2[j]; }
        }
        sum_waves_store_stat(red, stat, item);
    }
}

}  // namespace

bool conv_first_supported(const ustrun_src_t& s, int Cout) {
    return s.C <= CMAX && Cout == 64 && !s.pool && !s.scale && !s.relu && s.off_y == 0 && s.off_x == 0;
}
int conv_first_stat_rows(int N, int H, int W, int dtype) {
    if (dtype == USTRUN_D16 && (g_debug_flags & 16384)) return N * cdiv(H, MTH) * cdiv(W, MTW);
    return dtype == USTRUN_D16 ? conv_first_fwd_grid(N, conv_first_fwd_plan(N, H, W)) : N * cdiv(H, FTH) * cdiv(W, FTW);
}

int conv_first_fwd(const ustrun_src_t& s, const void* w_fwd, int dtype, int N, void* y, float* stat, hipStream_t st) {
    if (dtype == USTRUN_D16 && !(g_debug_flags & 16384)) {       // im2col on the matrix cores, streaming form (round 4)
        const CfFwdPlan plan = conv_first_fwd_plan(N, s.H, s.W);
        USTRUN_CHECK(s.C >= 1 && s.C <= CMAX, "conv_first_fwd: C=%d", s.C);
        const long img_elems = (long)(s.C - 1) * s.sC + (long)(s.H - 1) * s.sH + (long)(s.W - 1) * s.sW + 1;
        USTRUN_CHECK(img_elems * 4 < (1L << 31) && (long)s.H * s.W * 128 < (1L << 31), "conv_first_fwd: an image beyond 2^31 bytes");
        dim3 grid(conv_first_fwd_grid(N, plan)), block(256);
#define USTRUN_CFS(CC)                                                                                                              \
    do {                                                                                                                            \
        if (stat) hipLaunchKernelGGL((conv_first_fwd_stream_kernel<CC, true>), grid, block, 0, st, (const float*)s.ptr, (long)s.sN, (int)s.sC, \
                                     (int)s.sH, (int)s.sW, s.H, s.W, (const elt_t*)w_fwd, (elt_t*)y, stat, plan, (int)(img_elems * 4)); \
        else hipLaunchKernelGGL((conv_first_fwd_stream_kernel<CC, false>), grid, block, 0, st, (const float*)s.ptr, (long)s.sN, (int)s.sC,   \
                                (int)s.sH, (int)s.sW, s.H, s.W, (const elt_t*)w_fwd, (elt_t*)y, stat, plan, (int)(img_elems * 4));     \
    } while (0)
        if (s.C == 1) USTRUN_CFS(1); else if (s.C == 2) USTRUN_CFS(2); else if (s.C == 3) USTRUN_CFS(3); else USTRUN_CFS(4);
#undef USTRUN_CFS
        USTRUN_LAUNCH_CHECK("conv_first_fwd_stream");
        return 0;
    }
    if (dtype == USTRUN_D16) {            // the round-1..3 tile-per-block kernel (ustrun_debug_flags bit 14: A/B runs)
        const int tx = cdiv(s.W, MTW), ty = cdiv(s.H, MTH), ks = cdiv(9 * s.C, 16);
        dim3 grid(N * ty * tx), block(256);
#define USTRUN_CF(KS) hipLaunchKernelGGL(conv_first_fwd_mfma_kernel<KS>, grid, block, 0, st, (const float*)s.ptr, (long)s.sN, \
                                         (long)s.sC, (long)s.sH, (long)s.sW, s.C, s.H, s.W, (const elt_t*)w_fwd, (elt_t*)y, stat, tx, ty)
        if (ks == 1) USTRUN_CF(1); else if (ks == 2) USTRUN_CF(2); else USTRUN_CF(3);
#undef USTRUN_CF
        USTRUN_LAUNCH_CHECK("conv_first_fwd_mfma");
        return 0;
    }
    const int tx = cdiv(s.W, FTW), ty = cdiv(s.H, FTH);
    hipLaunchKernelGGL(conv_first_fwd_kernel, dim3(N * ty * tx), dim3(256), 0, st, (const float*)s.ptr, (long)s.sN, (long)s.sC,
                       (long)s.sH, (long)s.sW, s.C, s.H, s.W, (const float*)w_fwd, (float*)y, stat, tx, ty);
    USTRUN_LAUNCH_CHECK("conv_first_fwd");
    return 0;
}

int64_t conv_first_wgrad_partials_bytes() { return (int64_t)(CF_WG_ITEMS / CF_WG_WAVES) * 32 * 64 * sizeof(float); }

namespace {

int launch_reduce(const float* partials, int slabs, int C, float* dw, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(conv_first_wgrad_reduce_kernel, dim3(cdiv(64 * C * 9, 8)), dim3(1024), 0, st, partials, slabs, C, dw, accumulate);
    USTRUN_LAUNCH_CHECK("conv_first_wgrad_reduce");
    return 0;
}

// plan and launch the streaming kernel (the caller has asked conv_first_wgrad_stream_ok), then the slab reduce
template <typename Op>
int launch_wgrad_stream(const ustrun_src_t& s, const void* dy, int N, float* dw, int accumulate, float* partials, hipStream_t st,
                        const CfWgradBn bn = {}) {
    const CfWgradPlan p = conv_first_wgrad_plan(N, s.H, s.W);
    const auto kernel = conv_first_wgrad_stream_kernel<Op, 4>;
    if (Op::LDS > 65536) USTRUN_TRY(ensure_dynamic_lds((const void*)kernel, Op::LDS, Op::NAME));
    hipLaunchKernelGGL(kernel, dim3(p.blocks), dim3(256), Op::LDS, st, (const float*)s.ptr, (int)s.sN, (int)s.sC, (int)s.sH, s.C, s.H, s.W,
                       (int)((long)N * s.sN * 4), (const typename Op::dy_t*)dy, (int)((long)N * s.H * s.W * Op::PXB), partials, p.strips,
                       p.nseg, p.seg_rows, (int)p.items, bn);
    USTRUN_LAUNCH_CHECK(Op::NAME);
    return launch_reduce(partials, p.blocks, s.C, dw, accumulate, st);
}

}  // namespace

int conv_first_wgrad(const ustrun_src_t& s, const void* dy, int dy_esz, int N, float* dw, int accumulate, float* partials,
                     int64_t partials_bytes, hipStream_t st, bool x3) {
    USTRUN_CHECK(partials_bytes >= conv_first_wgrad_partials_bytes(), "conv_first_wgrad: partials too small");
    USTRUN_CHECK(dy_esz == (x3 ? 4 : 2), "conv_first_wgrad: %d-byte dY", dy_esz);
    const bool stream_ok = conv_first_wgrad_stream_ok(s, N, s.H, s.W, dy_esz);
    if (x3) {                           // dtype USTRUN_F32X3: f32 dY, three-term products
        USTRUN_CHECK(stream_ok, "conv_first_wgrad: layout outside the streaming kernel's range");
        return launch_wgrad_stream<WgOpX3>(s, dy, N, dw, accumulate, partials, st);
    }
    // (ustrun_debug_flags bit 28: the tile kernel of rounds 1-4, for A/B runs)
    if (stream_ok && !(g_debug_flags & (1 << 28))) return launch_wgrad_stream<WgOp16>(s, dy, N, dw, accumulate, partials, st);
    const int tx = cdiv(s.W, FTW), ty = cdiv(s.H, FTH), ttotal = N * ty * tx;
    int blocks = ttotal < 1024 ? ttotal : 1024;
    const int per = cdiv(ttotal, blocks);
    blocks = cdiv(ttotal, per);
    hipLaunchKernelGGL(conv_first_wgrad_kernel, dim3(blocks), dim3(256), 0, st, (const float*)s.ptr, (long)s.sN, (long)s.sC, (long)s.sH,
                       (long)s.sW, s.C, s.H, s.W, (const elt_t*)dy, partials, tx, ty, ttotal, per);
    USTRUN_LAUNCH_CHECK("conv_first_wgrad");
    return launch_reduce(partials, blocks, s.C, dw, accumulate, st);
}


// the 16-bit streaming weight gradient with layer 0's BatchNorm-backward apply pass on load (WgOp16Bn): dy = apply(da, y) is never stored
bool conv_first_wgrad_bn_ok(const ustrun_src_t& s, int N, int H, int W, int Cout, int dtype) {
    return dtype == USTRUN_D16 && conv_first_supported(s, Cout) && s.H == H && s.W == W && s.f32 && 9 * s.C <= 32 &&
           conv_first_wgrad_stream_ok(s, N, H, W, 2) && !(g_debug_flags & (1 << 28));
}
int conv_first_wgrad_bn(const ustrun_src_t& s, const void* da, const void* y, const float* scale, const float* shift, const float* coef,
                        int gN, long aff_stride, int N, float* dw, int accumulate, float* partials, int64_t partials_bytes,
                        hipStream_t st) {
    USTRUN_CHECK(da && y && scale && shift && coef && dw && partials, "conv_first_wgrad_bn: null pointer");
    USTRUN_CHECK(partials_bytes >= conv_first_wgrad_partials_bytes(), "conv_first_wgrad_bn: partials too small");
    USTRUN_CHECK(conv_first_wgrad_bn_ok(s, N, s.H, s.W, 64, USTRUN_D16), "conv_first_wgrad_bn: layout outside the streaming kernel's range");
    USTRUN_CHECK(gN >= 1 && aff_stride % 4 == 0 && !(((uintptr_t)scale | (uintptr_t)shift | (uintptr_t)coef) & 15),
                 "conv_first_wgrad_bn: constants must be 16-byte aligned, gN=%d", gN);
    const CfWgradBn bn = {y, scale, shift, coef, gN, (int)aff_stride, 3 * 64};
    return launch_wgrad_stream<WgOp16Bn>(s, da, N, dw, accumulate, partials, st, bn);
}

}  // namespace ustrun
