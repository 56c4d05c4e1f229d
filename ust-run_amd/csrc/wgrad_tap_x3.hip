// wgrad_tap_x3.hip -- dtype USTRUN_F32X3: weight gradient of a 1x1 / dilated / strided k x k convolution (k = 1, 3) with three-term
// bf16 products, one TAP per block (the DeepLabV2-ResNet bottlenecks, projection shortcuts, stem patches and classifier GEMM: every
// weight gradient the all-taps kernel of x3.hip -- undilated stride-1 3x3 only -- does not take):
//
//   dW[tap][ci][co] = sum_p act(x[stride * p + dilation * (tap - k/2)][ci]) * dy[p][co]          p over the output grid
//
// The tiling and the WgradArgs contract are wgrad_tap_bf16.hip's, the shared parts in tn_gemm.h.  The arithmetic is wgrad_x3_kernel's:
// both operands are f32 NHWC in HBM; a staged value goes global -> registers -> [BatchNorm affine + ReLU in f32, zero outside the
// image / the pixel range: x3_activate<true>] -> split3, store_planes -> three bf16 planes in LDS, [plane][pixel][channel]; a fragment pair
// is six MFMAs, smallest terms first, term by term over the wave's accumulators (x3_products, rows outer) -- all of x3_split.h.
//
// Stage = 32 pixels: LDS 3 planes x 32 x (TM + TN) x 2 B = 48 KB for the 128 x 128 tile, one buffer -- the loads of stage s + 1 are
// issued before the MFMAs of stage s and split into LDS after them; two blocks per CU (96 of 160 KB) cover each other's splits and
// barriers.  Per stage and wave (128 x 128): 48 MFMAs (1536 matrix-pipe cycles) against 24 transposing reads and ~320 VALU
// instructions of splitting per lane.
#include "common.h"
#include "loader.h"
#include "tn_gemm.h"
#include "x3_split.h"

namespace ustrun {
namespace {

constexpr int KP = 32;   // pixels per stage

// grid = (ci tiles * co tiles * taps * ksplit)
// SWAP (1x1 convolutions): the MFMA operands trade places, D rows are co and its lanes ci, so the slab comes out as [co][ci] --
// the torch layout of a 1x1 weight -- and the fixed-order streaming sum finishes it without a transposing pass.
template <int TM, int TN, bool SWAP>
__global__ __launch_bounds__(256, 2) void wgrad_tap_x3_kernel(const WgradArgs a, const int mtn, const int ntn) {
    constexpr int RBA = TM * 2, RBB = TN * 2;                 // LDS row pitches (bytes)
    constexpr int APLANE = KP * RBA, BPLANE = KP * RBB;       // one plane of a tile
    constexpr int AQ = TM / 4, AROWS = 256 / AQ, AP = KP / AROWS;      // 16-byte (4 x f32) items per row, rows per pass, passes
    constexpr int BQ = TN / 4, BROWS = 256 / BQ, BP = KP / BROWS;
    constexpr int MI = TM / 64, NI = TN / 64;                 // 32 x 32 MFMA tiles per wave (waves 2 x 2)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                      // [3][KP][TM] bf16
    char* Bs = smem + 3 * APLANE;         // [3][KP][TN] bf16

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nblk = gridDim.x, tiles = nblk / a.ksplit;
    // (block decode and slab epilogue stay local in both one-tap kernels: as shared functions they changed the kernels' instructions)
    const int lin = xcd_linear(blockIdx.x, nblk);
    const int ks = lin / tiles;
    int tile = lin - ks * tiles;
    const int ntile = tile % ntn; tile /= ntn;
    const int mtile = tile % mtn;
    const int seg = tile / mtn;
    const int ci0 = mtile * TM, co0 = ntile * TN;
    const int ady = a.d0 + (seg / a.segw) * a.astep, adx = a.d0 + (seg % a.segw) * a.astep;
    const int kbeg = (int)((long)ks * a.kchunk);
    const int kend = (kbeg + a.kchunk < a.M) ? (int)(kbeg + a.kchunk) : (int)a.M;
    const int Wb = a.Wb, Hb = a.Hb;
    const float invW = 1.f / (float)Wb, invH = 1.f / (float)Hb;

    // ---- activation items: pixel row tid / AQ + AROWS i of the stage, 4-channel group tid % AQ ----
    const SrcDev& S = a.src[0];
    const int c4 = tid % AQ, arow = tid / AQ;
    const int cl = ci0 + 4 * c4;
    f32x4 asc = {1.f, 1.f, 1.f, 1.f}, ash = {0.f, 0.f, 0.f, 0.f};
    if (S.scale) { asc = *(const f32x4*)(S.scale + cl); ash = *(const f32x4*)(S.shift + cl); }
    const float floor_ = x3_floor(S.relu);
    const float* sp = S.ptr + cl;
    const int sN = (int)S.sN, sH = (int)S.sH, sW = (int)S.sW;        // element offsets fit 31 bits (host check)
    f32x4 av[AP];
    unsigned aok = 0;
    // every load is issued unconditionally from an in-range address (the source's first pixel for rows outside the pixel range /
    // the image) and the row is zeroed at the split: no load is ever addressed outside the tensor
    auto load_A = [&](int k0) {
        aok = 0;
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const int m = k0 + arow + AROWS * i;
            int px, py;
            const int r = fdiv(m < kend ? m : kbeg, Wb, invW, px);
            const int pn = fdiv(r, Hb, invH, py);
            const int ly = (py << a.ashift) + ady - S.off_y, lx = (px << a.ashift) + adx - S.off_x;
            const int ok = (int)(m < kend) & (int)((unsigned)ly < (unsigned)S.LH) & (int)((unsigned)lx < (unsigned)S.LW);
            const int off = pn * sN + ly * sH + lx * sW;
            av[i] = *(const f32x4*)(sp + (ok ? off : 0));
            aok |= (unsigned)ok << i;
        }
    };
    auto write_A = [&]() {
#pragma unroll
        for (int i = 0; i < AP; ++i) {
            const int row = arow + AROWS * i;
            // BatchNorm affine + ReLU in f32, then padding / the range's tail, before the split
            store_planes(split3(x3_activate<true>(av[i], asc, ash, floor_, (aok >> i) & 1u)), As + row * RBA + ((c4 * 8) ^ (seg_swz<RBA>(row) << 6)), APLANE);
        }
    };
    // ---- dy items: the same (row, 4-channel group) pattern over pixel-linear rows of Cout floats ----
    const int b4 = tid % BQ, brow = tid / BQ;
    const float* dyp = a.dy + co0 + 4 * b4;
    const int dyC = a.Cout;
    f32x4 bv[BP];
    auto load_B = [&](int k0) {
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            const int m = k0 + brow + BROWS * i;
            bv[i] = *(const f32x4*)(dyp + (m < kend ? m : kbeg) * dyC);      // (rows past the range: an in-range pixel, zeroed below)
        }
    };
    auto write_B = [&](int k0) {
#pragma unroll
        for (int i = 0; i < BP; ++i) {
            const int row = brow + BROWS * i;
            const f32x4 v = (k0 + row < kend) ? bv[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
            store_planes(split3(v), Bs + row * RBB + ((b4 * 8) ^ (seg_swz<RBB>(row) << 6)), BPLANE);
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (kbeg < kend) {
        load_A(kbeg);
        load_B(kbeg);
        write_A();
        write_B(kbeg);
    }
    __syncthreads();
#pragma unroll 1
    for (int k0 = kbeg; k0 < kend; k0 += KP) {
        const bool more = k0 + KP < kend;
        if (more) {                                   // in flight under this stage's MFMAs
            load_A(k0 + KP);
            load_B(k0 + KP);
        }
#pragma unroll
        for (int kk = 0; kk < KP / 16; ++kk) {
            b16x8 af[MI][3], bf[NI][3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
#pragma unroll
                for (int i = 0; i < MI; ++i) af[i][p] = tr_frag<RBA, __bf16>(As + p * APLANE, kk * 16, wm * (TM / 2) + 32 * i, lane);
#pragma unroll
                for (int j = 0; j < NI; ++j) bf[j][p] = tr_frag<RBB, __bf16>(Bs + p * BPLANE, kk * 16, wn * (TN / 2) + 32 * j, lane);
            }
            x3_products<false, SWAP>(af, bf, acc);        // term by term: an accumulator's products stand MI * NI instructions apart
        }
        __syncthreads();                              // every wave is done reading this stage
        if (more) {
            write_A();
            write_B(k0 + KP);
        }
        __syncthreads();
    }

    float* slab = a.partials + ((long)ks * a.nseg + seg) * a.Cin * a.Cout;
    const int l31 = lane & 31, lh = lane >> 5;
    if (SWAP) {
        // slab [ks][Cout][Cin]: rows of D are co (registers), the 32 lanes of a row are consecutive ci
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int ci = ci0 + wm * (TM / 2) + i * 32 + l31;
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + wn * (TN / 2) + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    slab[(long)co * a.Cin + ci] = acc[i][j][r];
                }
        }
    } else {
        // slab [ks][tap][Cin][Cout]: rows of D are ci (registers), the 32 lanes of a row are consecutive co
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int co = co0 + wn * (TN / 2) + j * 32 + l31;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ci = ci0 + wm * (TM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    slab[(long)ci * a.Cout + co] = acc[i][j][r];
                }
        }
    }
}

template <int TM, int TN>
int launch_tile(const WgradArgs& a, hipStream_t st) {
    const int mtn = a.Cin / TM, ntn = a.Cout / TN;
    dim3 grid(mtn * ntn * a.nseg * a.ksplit), block(256);
    constexpr int lds = 3 * KP * (TM + TN) * 2;               // <= 48 KB
    if (a.nseg == 1) hipLaunchKernelGGL((wgrad_tap_x3_kernel<TM, TN, true>), grid, block, lds, st, a, mtn, ntn);
    else hipLaunchKernelGGL((wgrad_tap_x3_kernel<TM, TN, false>), grid, block, lds, st, a, mtn, ntn);
    USTRUN_LAUNCH_CHECK("wgrad_tap_x3");
    return 0;
}

}  // namespace

bool wgrad_tap_x3_supported(const WgradArgs& a) {
    if (g_debug_flags & X3_DBG_OFF) return false;                  // (A/B runs against the f32 matrix-core kernel)
    if (a.dy_s != 1 || a.dy_esz != 4 || a.nsrc != 1 || a.ashift < 0 || a.ashift > 1 || a.astep < 1) return false;
    if (!((a.nseg == 1 && a.segw == 1) || (a.nseg == 9 && a.segw == 3))) return false;      // k = 1 or 3
    const SrcDev& s = a.src[0];
    if (!x3_src_ok(s) || s.gN > 0 || s.C != a.Cin) return false;
    if (a.dyH != a.Hb || a.dyW != a.Wb || a.M <= 0 || a.M >= (1L << 24)) return false;      // float-reciprocal pixel decomposition
    if ((long)a.N * s.sN >= (1L << 31) - 64 || a.M * a.Cout >= (1L << 31) - 64) return false;      // 32-bit element offsets
    return a.Cin % 64 == 0 && a.Cout % 64 == 0;
}

int wgrad_tap_x3_plan(const WgradArgs& a, int* ksplit, long* kchunk) { return tap_plan(a, KP, ksplit, kchunk); }

int wgrad_tap_x3_launch(const WgradArgs& a, hipStream_t st) {
    const int tm = tap_tile_m(a), tn = tap_tile_n(a);
    // 'X' | TM/64 | TN/64 | slab layout (1 = one tap, [co][ci]; 0 = k x k taps, [tap][ci][co]) | ksplit   (tests: ustrun_debug_last_wgrad_variant)
    set_last_wgrad_variant(0x58000000 | (tm / 64) << 20 | (tn / 64) << 16 | (a.nseg == 1 ? 1 : 0) << 12 | (a.ksplit & 0xfff));
    if (tm == 128 && tn == 128) return launch_tile<128, 128>(a, st);
    if (tm == 128) return launch_tile<128, 64>(a, st);
    if (tn == 128) return launch_tile<64, 128>(a, st);
    return launch_tile<64, 64>(a, st);
}

}  // namespace ustrun
