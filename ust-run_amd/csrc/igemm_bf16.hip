// igemm_bf16.hip -- the implicit-GEMM kernel of igemm.hip on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16, f32 accumulate).  Activations stay f32 in HBM this round: the loader
// applies the BatchNorm/ReLU/pool/concat transform in f32, rounds to bf16 (RNE) and stores a
// K-contiguous, XOR-swizzled A tile in LDS; weights are pre-packed in bf16 as [slice][K/8][N][8] so
// that a lane's 8 consecutive K values are one 16-byte LDS read with no conflicts.
#include "igemm_tile.h"

namespace ustrun {
namespace {

template <int WM, int WN, bool POOL>
__global__ __launch_bounds__(256, 2) void igemm_bf16_kernel(const IgemmArgs a, const int mt_total, const int nt_total) {
    constexpr int BM = WM * 64, BN = WN * 64;
    constexpr int BK = POOL ? 32 : 64;
    constexpr int CPR = BK / 4;            // 4-channel groups per row
    constexpr int RPP = 256 / CPR;         // rows per pass
    constexpr int AR = BM / RPP;           // rows per thread per stage
    constexpr int NP = POOL ? 4 : 1;
    constexpr int ROWB = BK * 2;           // bytes per A row in LDS
    constexpr int BCH = (BK / 8) * BN;     // 16-byte chunks in the B tile
    constexpr int BR = BCH / 256;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                        // [BM][BK] bf16, 16-B chunks XOR-swizzled by row
    char* Bs = smem + BM * ROWB;            // [BK/8][BN][8] bf16
    RowInfo* rowinfo = (RowInfo*)(Bs + BCH * 16);

    const int bid = xcd_linear(blockIdx.x, mt_total * nt_total);
    const int mtile = bid / nt_total, ntile = bid % nt_total;
    const int z = blockIdx.y;
    const int n0 = ntile * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    fill_row_table<BM>(rowinfo, a, mtile, tid);

    auto swz = [](int row) { return BK == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3); };

    const int a_c4 = tid % CPR, a_r0 = tid / CPR;
    const bool vecA = sources_vectorizable(a.src[0], a.src[1], a.nsrc, 2);
    const int nchunk = (a.Cin + BK - 1) / BK;
    const int nstage = a.nseg * nchunk;
    const int K8 = (a.Cin + 7) / 8;         // packed K octets per slice
    const elt_t* Wp = (const elt_t*)a.W;

    f32x4 av[AR][NP], asc, ash;
    unsigned aok;
    int a_relu;
    bf16x8 bv[BR];

    auto load_stage = [&](int s) {
        const int seg = s / nchunk, c0 = (s - seg * nchunk) * BK;
        load_a_stage<2, POOL, AR, RPP>(av, asc, ash, a_relu, aok, a, rowinfo, vecA, seg, c0 + 4 * a_c4, a_r0);
        // B tile: packed bf16 weights [slice][K8][Cout][8]
        const elt_t* wb = Wp + ((long)(seg + z) * K8) * a.Cout * 8;
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const int idx = tid + 256 * i, o = idx / BN, n = idx % BN;
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (elt_t)0.f;
            const int ko = c0 / 8 + o;
            if (ko < K8 && n0 + n < a.Cout) v = *(const bf16x8*)(wb + ((long)ko * a.Cout + n0 + n) * 8);
            bv[i] = v;
        }
    };

    auto write_stage = [&]() {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const f32x4 v = activate(av[i], asc, ash, a_relu, (aok >> i) & 1u, vecA);
            const int row = a_r0 + RPP * i;
            bf16x4 h;
            h[0] = (elt_t)v[0]; h[1] = (elt_t)v[1]; h[2] = (elt_t)v[2]; h[3] = (elt_t)v[3];
            *(bf16x4*)(As + row * ROWB + (((a_c4 >> 1) ^ swz(row)) * 16) + (a_c4 & 1) * 8) = h;
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) *(bf16x8*)(Bs + (tid + 256 * i) * 16) = bv[i];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;
    const int rowA = wm * 64 + l31;
    const char* Ap0 = As + rowA * ROWB;
    const char* Ap1 = As + (rowA + 32) * ROWB;
    const int sw0 = swz(rowA), sw1 = swz(rowA + 32);
    const char* Bp = Bs + (lh * BN + wn * 64 + l31) * 16;

    load_stage(0);
    for (int s = 0; s < nstage; ++s) {
        write_stage();
        __syncthreads();
        if (s + 1 < nstage) load_stage(s + 1);
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            const int ch = 2 * ks + lh;
            const bf16x8 a0 = *(const bf16x8*)(Ap0 + ((ch ^ sw0) * 16));
            const bf16x8 a1 = *(const bf16x8*)(Ap1 + ((ch ^ sw1) * 16));
            const bf16x8 b0 = *(const bf16x8*)(Bp + (2 * ks * BN) * 16);
            const bf16x8 b1 = *(const bf16x8*)(Bp + (2 * ks * BN + 32) * 16);
            acc[0][0] = USTRUN_MFMA_32x32x16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = USTRUN_MFMA_32x32x16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = USTRUN_MFMA_32x32x16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = USTRUN_MFMA_32x32x16(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    igemm_epilogue<WM, WN, true>(a, acc, rowinfo, (float*)As, mtile, n0, z, tid);
}

template <int WM, int WN, bool POOL>
int launch_cfg(const IgemmArgs& a, hipStream_t st) {
    constexpr int BM = WM * 64, BN = WN * 64, BK = POOL ? 32 : 64;
    const int mt = cdiv(a.M, BM), nt = cdiv(a.Cout, BN);
    const size_t lds = (size_t)BM * BK * 2 + (size_t)BK * BN * 2 + (size_t)BM * sizeof(RowInfo);
    dim3 grid(mt * nt, a.nz), block(256);
    hipLaunchKernelGGL((igemm_bf16_kernel<WM, WN, POOL>), grid, block, lds, st, a, mt, nt);
    USTRUN_LAUNCH_CHECK("igemm_bf16");
    return 0;
}

// torch conv weight [Cout][Cin][taps] (taps = 9) or convT weight [Cin][Cout][taps] (taps = 4)
// -> fwd [tap][ceil(Cin/8)][Cout][8] and dgrad [tap][ceil(Cout/8)][Cin][8], bf16, zero padded
__global__ void pack_bf16_kernel(const float* __restrict__ w, int Cout, int Cin, int taps, int transposed_src,
                                 elt_t* __restrict__ wf, elt_t* __restrict__ wd) {
    const int Ki = (Cin + 7) / 8, Ko = (Cout + 7) / 8;
    const long nf = (long)taps * Ki * Cout * 8, nd = (long)taps * Ko * Cin * 8;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nf + nd; e += (long)gridDim.x * blockDim.x) {
        int tap, ci, co;
        if (e < nf) {
            const int j = (int)(e & 7); long t = e >> 3;
            co = (int)(t % Cout); t /= Cout;
            ci = (int)(t % Ki) * 8 + j; tap = (int)(t / Ki);
        } else {
            const long f = e - nf;
            const int j = (int)(f & 7); long t = f >> 3;
            ci = (int)(t % Cin); t /= Cin;
            co = (int)(t % Ko) * 8 + j; tap = (int)(t / Ko);
        }
        float v = 0.f;
        if (ci < Cin && co < Cout)
            v = transposed_src ? w[((long)ci * Cout + co) * taps + tap] : w[((long)co * Cin + ci) * taps + tap];
        if (e < nf) wf[e] = (elt_t)v; else if (wd) wd[e - nf] = (elt_t)v;
    }
}

}  // namespace

int igemm_launch_bf16(const IgemmArgs& a, hipStream_t st) {
    const IgemmTile tile = igemm_pick_tile(a);
    if (tile.wm == 2) return tile.pool ? launch_cfg<2, 2, true>(a, st) : launch_cfg<2, 2, false>(a, st);
    return launch_cfg<4, 1, false>(a, st);
}

// all layers of a model in one launch: blockIdx.y = layer.  A thread owns one (co, ci) pair of the K/N-padded grid:
// it reads the pair's `taps` consecutive source floats (threads run along the source's inner index: coalesced) and
// scatters them to the tap planes of both packed layouts.  (One thread per OUTPUT element re-fetched every source line
// once per tap: 1.3 GB moved for 250 MB.)
__global__ __launch_bounds__(256) void pack_bf16_multi_kernel(const PackJobs jobs) {
    const PackJob j = jobs.j[blockIdx.y];
    const float* __restrict__ w = j.w;
    elt_t* wf = (elt_t*)j.wf;
    elt_t* wd = (elt_t*)j.wd;
    const int Cin = j.Cin, Cout = j.Cout, taps = j.taps;
    // 3x3 conv weights with whole 64-channel input groups (every layer but the first): a block takes 8 output channels
    // x 64 input channels -- 8 contiguous 2304-byte runs of the source -- through LDS and writes both layouts in
    // 16-byte pieces that add up to whole 128-byte (forward) and 1 KB (input-gradient) runs.  The element-per-thread
    // path below wrote 2-byte pieces 16 bytes apart: 1.3 GB of HBM traffic for 248 MB of weights.
    if (!j.transposed_src && taps == 9 && Cin % 64 == 0 && Cout % 8 == 0 && wd) {
        __shared__ elt_t t[8][64 * 9 + 2];                 // [co][ci*9 + tap] (+2: rows start 4 bytes apart in the banks)
        const int Ki = Cin / 8, Ko = Cout / 8, tiles_ci = Cin / 64, ntile = Ko * tiles_ci;
        for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
            const int cog = tile / tiles_ci, ci0 = (tile % tiles_ci) * 64;
            __syncthreads();
            for (int e = threadIdx.x; e < 8 * 144; e += 256) {          // 144 float4 per output channel
                const int co = e / 144, q = e % 144;
                const f32x4 v = *(const f32x4*)(w + ((long)(cog * 8 + co) * Cin + ci0) * 9 + 4 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) t[co][4 * q + k] = (elt_t)v[k];
            }
            __syncthreads();
            for (int e = threadIdx.x; e < 9 * 8 * 8; e += 256) {        // forward: (tap, ci group, co) -> 8 ci
                const int co = e & 7, cig = (e >> 3) & 7, tap = e >> 6;
                bf16x8 v;
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t[co][(cig * 8 + k) * 9 + tap];
                *(bf16x8*)(wf + (((long)tap * Ki + ci0 / 8 + cig) * Cout + cog * 8 + co) * 8) = v;
            }
            for (int e = threadIdx.x; e < 9 * 64; e += 256) {           // input gradient: (tap, ci) -> 8 co
                const int ci = e & 63, tap = e >> 6;
                bf16x8 v;
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t[k][ci * 9 + tap];
                *(bf16x8*)(wd + (((long)tap * Ko + cog) * Cin + ci0 + ci) * 8) = v;
            }
        }
        return;
    }
    const int Ki = (Cin + 7) / 8, Ko = (Cout + 7) / 8;
    const int Pi = Ki * 8, Po = Ko * 8;
    const long total = (long)Pi * Po;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        int ci, co;
        if (j.transposed_src) { co = (int)(e % Po); ci = (int)(e / Po); }       // source [Cin][Cout][taps]
        else { ci = (int)(e % Pi); co = (int)(e / Pi); }                        // source [Cout][Cin][taps]
        const bool in = ci < Cin && co < Cout;
        const float* src = w + (j.transposed_src ? ((long)ci * Cout + co) : ((long)co * Cin + ci)) * taps;
        for (int tap = 0; tap < taps; ++tap) {
            const elt_t v = (elt_t)(in ? src[tap] : 0.f);
            if (co < Cout) wf[(((long)tap * Ki + ci / 8) * Cout + co) * 8 + (ci & 7)] = v;
            if (wd && ci < Cin) wd[(((long)tap * Ko + co / 8) * Cin + ci) * 8 + (co & 7)] = v;
        }
    }
}

int pack_bf16_multi(const PackJobs& jobs, int n, hipStream_t st) {
    hipLaunchKernelGGL(pack_bf16_multi_kernel, dim3(1024, n), dim3(256), 0, st, jobs);   // small layers: most blocks exit at once
    USTRUN_LAUNCH_CHECK("pack_bf16_multi");
    return 0;
}

int pack_bf16(const float* w, int Cout, int Cin, int taps, int transposed_src, void* wf, void* wd, hipStream_t st) {
    const long total = (long)taps * (((Cin + 7) / 8) * (long)Cout + ((Cout + 7) / 8) * (long)Cin) * 8;
    long b = (total + 1023) / 1024;
    if (b > 4096) b = 4096;
    hipLaunchKernelGGL(pack_bf16_kernel, dim3((int)b), dim3(256), 0, st, w, Cout, Cin, taps, transposed_src, (elt_t*)wf,
                       (elt_t*)wd);
    USTRUN_LAUNCH_CHECK("pack_bf16");
    return 0;
}

}  // namespace ustrun
