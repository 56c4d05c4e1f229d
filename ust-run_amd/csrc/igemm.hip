// igemm.hip -- generic implicit-GEMM kernel on the exact-f32 matrix cores of gfx950.
//
//   out[map_out(m)][n] = bias[n] + sum_{seg} sum_{c} A_seg[m][c] * W[seg][c][n]
//
// m runs over a base pixel grid (N,Hb,Wb); A_seg[m][c] is the loader's view of the activation
// sources at pixel base*s_in + (dy,dx)_seg (BatchNorm affine + ReLU, 2x2 max-pool, concat of two
// sources and zero padding are all evaluated on the fly, never materialised); W is the packed
// weight [slice][Cin][Cout].  conv3x3 forward / input-gradient use 9 segments, ConvTranspose
// forward uses 4 output parity classes (grid.z) with one segment each, its input-gradient 4
// segments with s_in = 2.
//
// Tile: 256 threads = 4 waves, each wave owns a 64x64 output tile as 2x2 v_mfma_f32_32x32x2_f32
// accumulators (bitwise an f32 fmaf chain, MI355X_MICROARCH "Matrix cores").  K is consumed in
// stages of 32 channels: global -> registers (prefetched under the previous stage's MFMAs) ->
// transform -> LDS (A stored k-major so that lanes read consecutive pixels, B row-major) -> MFMA.
#include "igemm_tile.h"
#include "convT_plan.h"
#include <stdlib.h>

namespace ustrun {

namespace {

constexpr int BK = 32;

template <int WM, int WN, bool POOL>
__global__ __launch_bounds__(256, 2) void igemm_f32_kernel(const IgemmArgs a, const int mt_total, const int nt_total) {
    constexpr int BM = WM * 64, BN = WN * 64;
    constexpr int LDA = BM + 1;
    constexpr int AR = BM / 32;         // A rows per thread per stage
    constexpr int NP = POOL ? 4 : 1;    // stored pixels per logical pixel
    constexpr int BQ = BN / 4;          // float4 per B row
    constexpr int BPASS = 256 / BQ;     // B rows covered per pass
    constexpr int BR = BK / BPASS;      // B float4 per thread per stage
    constexpr int A_FLOATS = (BK * LDA + 3) & ~3;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* As = (float*)smem;
    float* Bs = As + A_FLOATS;
    RowInfo* rowinfo = (RowInfo*)(Bs + BK * BN);

    // XCD-aware tile id: n-tiles of one m-tile adjacent -> A panel shared in the XCD's L2
    const int bid = xcd_linear(blockIdx.x, mt_total * nt_total);
    const int mtile = bid / nt_total, ntile = bid % nt_total;
    const int z = blockIdx.y;
    const int n0 = ntile * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    fill_row_table<BM>(rowinfo, a, mtile, tid);

    const int a_c4 = tid & 7, a_r0 = tid >> 3;
    const int b_n4 = tid % BQ, b_k0 = tid / BQ;
    const bool vecA = sources_vectorizable(a.src[0], a.src[1], a.nsrc);
    const bool vecB = (a.Cout & 3) == 0;
    const int nchunk = (a.Cin + BK - 1) / BK;
    const int nstage = a.nseg * nchunk;

    f32x4 av[AR][NP], asc, ash;
    unsigned aok;
    int a_relu;
    f32x4 bv[BR];

    auto load_stage = [&](int s) {
        const int seg = s / nchunk, c0 = (s - seg * nchunk) * BK;
        load_a_stage<4, POOL, AR, 32>(av, asc, ash, a_relu, aok, a, rowinfo, vecA, seg, c0 + 4 * a_c4, a_r0);
        // B tile: W[slice][c0 + k][n0 + 4*b_n4 ..]
        const float* wb = a.W + ((long)(seg + z) * a.Cin) * a.Cout;
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const int k = c0 + b_k0 + BPASS * i, n = n0 + 4 * b_n4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < a.Cin) {
                const float* p = wb + (long)k * a.Cout + n;
                if (vecB) { if (n < a.Cout) v = *(const f32x4*)p; }
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (n + j < a.Cout) v[j] = p[j];
                }
            }
            bv[i] = v;
        }
    };

    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const f32x4 v = activate(av[i], asc, ash, a_relu, (aok >> i) & 1u, vecA);
            const int row = a_r0 + 32 * i;
#pragma unroll
            for (int j = 0; j < 4; ++j) As[(4 * a_c4 + j) * LDA + row] = v[j];
        }
#pragma unroll
        for (int i = 0; i < BR; ++i)
            *(f32x4*)(Bs + (b_k0 + BPASS * i) * BN + 4 * b_n4) = bv[i];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;
    const float* Ap = As + lh * LDA + wm * 64 + l31;
    const float* Bp = Bs + lh * BN + wn * 64 + l31;

    load_stage(0);
    for (int s = 0; s < nstage; ++s) {
        write_stage();
        __syncthreads();
        if (s + 1 < nstage) load_stage(s + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const float a0 = Ap[2 * kk * LDA], a1 = Ap[2 * kk * LDA + 32];
            const float b0 = Bp[2 * kk * BN], b1 = Bp[2 * kk * BN + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    igemm_epilogue<WM, WN, false>(a, acc, rowinfo, As, mtile, n0, z, tid);
}

template <int WM, int WN, bool POOL>
int launch_cfg(const IgemmArgs& a, hipStream_t st) {
    constexpr int BM = WM * 64, BN = WN * 64;
    const int mt = cdiv(a.M, BM), nt = cdiv(a.Cout, BN);
    const size_t lds = (size_t)(((BK * (BM + 1) + 3) & ~3) + BK * BN) * 4 + (size_t)BM * sizeof(RowInfo);
    dim3 grid(mt * nt, a.nz), block(256);
    hipLaunchKernelGGL((igemm_f32_kernel<WM, WN, POOL>), grid, block, lds, st, a, mt, nt);
    USTRUN_LAUNCH_CHECK("igemm");
    return 0;
}

}  // namespace

// one statistics row per 128 pixels (igemm_epilogue) whatever Cout and the tile it selects: the parameter stays for the callers
int igemm_mtiles(int64_t M, int) { return cdiv(M, 128); }

// stat rows actually written by the kernel igemm_launch will pick
int igemm_stat_rows_used(const IgemmArgs& a, int dtype) {
    if (dtype == USTRUN_D16 && !(g_debug_flags & 1) && ws64_supported(a)) return ws64_stat_rows(a);
    if (dtype == USTRUN_D16 && halo_supported(a)) return halo_stat_rows_used(a);
    if (dtype == USTRUN_F32X3 && conv3x3_x3_supported(a)) return conv3x3_x3_stat_rows(a);
    if (const ConvTPlan tp = convT_plan(a, g_debug_flags); dtype == USTRUN_D16 && tp.kind != CONVT_NONE) return tp.stat_rows;
    return cdiv(a.M, 128);
}

int igemm_launch(const IgemmArgs& a, int dtype, hipStream_t st) {
    USTRUN_CHECK(dtype_ok(dtype), "igemm: dtype %d not built", dtype);
    USTRUN_CHECK(a.M > 0 && a.Cout > 0 && a.Cin > 0, "igemm: empty problem");
    USTRUN_CHECK(a.Hb < 65536 && a.Wb < 65536, "igemm: extent too large");
    USTRUN_CHECK(a.nseg >= 1 && a.nseg <= 49 && a.nz >= 1 && a.nz <= 4, "igemm: bad segment/parity count");
    int csum = 0;
    for (int i = 0; i < a.nsrc; ++i) csum += a.src[i].C;
    const IgemmTile tile = igemm_pick_tile(a);
    USTRUN_CHECK(csum == a.Cin, "igemm: source channels %d != Cin %d", csum, a.Cin);
    USTRUN_CHECK(!tile.pool || a.nsrc == 1, "igemm: pooled source cannot be concatenated");
    // algorithmic cost of this launch: every stored input/weight/output element touched once
    double in_elems = 0;
    for (int i = 0; i < a.nsrc; ++i) in_elems += (double)a.N * a.src[i].H * a.src[i].W * a.src[i].C;
    const double out_elems = (double)a.M * a.nz * a.Cout;
    const double w_elems = (double)a.nseg * a.nz * a.Cin * a.Cout;
    const double aesz = dtype == USTRUN_D16 ? 2.0 : 4.0;     // stored element size of activations and packed weights
    // (an input gradient that also forms the BatchNorm-backward sums reads y beside every output element it stores)
    const double y_elems = (a.bny ? out_elems : 0.0) + (a.join_add ? out_elems : 0.0) + (a.join_ref ? out_elems : 0.0);
    prof_begin(0, 2.0 * a.M * a.nz * a.Cout * a.nseg * a.Cin, aesz * (in_elems + out_elems + y_elems + w_elems), st);
    int rc;
    bool grouped = false;
    for (int i = 0; i < a.nsrc; ++i) grouped |= a.src[i].gN > 0;
    USTRUN_CHECK(!grouped || dtype == USTRUN_D16 || (dtype == USTRUN_F32X3 && conv3x3_x3_supported(a)),
                 "igemm: batched passes reached a kernel without per-pass BatchNorm constants");
    if (dtype == USTRUN_D16) {
        const ConvTPlan tp = convT_plan(a, g_debug_flags);      // the pixel-linear GEMM family (convT_plan.h): asked once
        if ((a.join_add || a.join_ref) && !tp.join) { set_error("conv1x1_join: unsupported shape"); rc = 1; }
        else if (!(g_debug_flags & 1) && ws64_supported(a)) rc = conv3x3_ws64_launch_bf16(a, st);
        else if (halo_supported(a)) rc = conv3x3_halo_launch_bf16(a, st);
        else if (tp.kind != CONVT_NONE) rc = convT_launch_bf16(a, tp, st);
        else if (grouped) { set_error("igemm: batched passes reached a kernel without per-pass BatchNorm constants"); rc = 1; }
        else rc = igemm_launch_bf16(a, st);
    } else if (dtype == USTRUN_F32X3 && igemm_x3_supported(a) && (!grouped || conv3x3_x3_supported(a))) {     // three-term bf16 products (x3.hip)
        rc = igemm_x3_launch(a, st);
    } else if (tile.wm == 2) {
        rc = tile.pool ? launch_cfg<2, 2, true>(a, st) : launch_cfg<2, 2, false>(a, st);
    } else {
        rc = launch_cfg<4, 1, false>(a, st);
    }
    prof_end(st);
    return rc;
}

}  // namespace ustrun
