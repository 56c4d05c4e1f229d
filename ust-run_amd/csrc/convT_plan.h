// convT_plan.h -- the plan of the pixel-linear GEMM family: convT_bf16.hip (ConvTranspose2d(k=2,s=2) forward, its input gradient, the 1x1
// convolution with its optional residual join and BatchNorm-backward sums) and wgradT_bf16.hip (the ConvTranspose weight + bias gradient,
// round-1 and round-5 kernel).  As halo_plan.h: the geometry of a build (ConvTGeom, T2: read by the kernel and by its launch), the list of
// builds (CONVT_BUILDS, WGRADT_BUILDS: what the dispatch instantiates, in the order the kernels lie in the code object), and the ONE
// decision per launch (convT_plan, wgradT_plan: kind, build, tiles, grid, LDS bytes, statistics rows, split-K, the variant code the tests
// read).  Pure host integer code: tests/host/convT_plan_check.hip compiles it for the host and pins it over a sweep of shapes and flags.
#pragma once
#include "common.h"

namespace ustrun {

// ---- the bits of ustrun_debug_flags this plan reads (A/B runs and the tests that pin the flag-only builds) ----
constexpr int CONVT_DBG_LDS_WEIGHTS = 512;          // bit 9: the round-2 builds with weight tiles in LDS (register-fed weights off)
constexpr int WGRADT_DBG_ROUND1 = 1 << 27;          // bit 27: the weight gradient never on the round-5 kernel

// the code ustrun_debug_last_conv_variant reports: 'CT' | join | join with sums | register-fed weights | BN/32 | BK/32 | MODE
constexpr int convT_variant(int BN, int BK, int MODE, bool BREG, bool BNS, bool JOIN) {
    return 0x43540000 | (JOIN ? 0x4000 : 0) | (JOIN && BNS ? 0x2000 : 0) | (BREG ? 0x1000 : 0) | (BN / 32) << 8 | (BK / 32) << 4 | MODE;
}
// a build's key: the variant code and, above it, what the code leaves out (the gradient's sums)
constexpr long convT_key(int BN, int BK, int MODE, bool BREG, bool BNS, bool JOIN) {
    return (long)(BNS ? 1 : 0) << 32 | convT_variant(BN, BK, MODE, BREG, BNS, JOIN);
}
// ---- geometry of one build of convT_bf16_kernel, over its template parameters.  MODE 0: forward, 1: input gradient, 2: 1x1 ----
template <int TBN, int TBK, int MODE, bool BREG, bool BNS = false, bool JOIN = false>
struct ConvTGeom {
    static constexpr int BN = TBN, BK = TBK, BM = 128;  // columns per tile, K per chunk, pixels per tile = pixels per statistics row
    static_assert(!BNS || MODE == 1 || JOIN, "BatchNorm-backward sums ride on an input gradient's epilogue");
    static_assert(!JOIN || MODE == 2, "the residual join rides on the 1x1 GEMM");
    static_assert(!BREG || BK == 64, "register-fed weights: two stages of two k-steps per chunk");
    static constexpr int WN = BN / 64, WM = 4 / WN, MI = BM / (32 * WM);
    static constexpr int CPR = BK / 8;                  // 16-byte groups per pixel per chunk
    static constexpr int AIT = BM * CPR / 256;          // A items per thread per chunk
    static constexpr int ROWB = BK * 2, ABYTES = BM * ROWB;
    static constexpr int BCH = CPR * BN, BIT = BCH / 256;   // 16-byte chunks per B tile
    static_assert(BCH % 256 == 0 && 256 % BN == 0, "B tile mapping: a thread keeps one column");
    static constexpr int EPITCH = 144, EPBYTES = 4 * 32 * EPITCH;     // the epilogue's per-wave transposition scratch
    // dynamic LDS: 2 x activation tile; 2 x weight tile, or none with BREG (the epilogue scratch aliases the tiles)
    static constexpr int lds = BREG ? (2 * ABYTES > EPBYTES ? 2 * ABYTES : EPBYTES) : 2 * ABYTES + 2 * BCH * 16;
    static constexpr int variant = convT_variant(BN, BK, MODE, BREG, BNS, JOIN);
};
constexpr int CONVT_BM = 128;
// ---- the builds: X(BN, BK, MODE, BREG, BNS, JOIN), in the order the dispatch instantiates them ----
#define CONVT_BUILDS(X) \
    X(256, 32, 0, 0, 0, 0) X(256, 64, 0, 1, 0, 0)                                                        /* forward */ \
    X(256, 32, 2, 0, 0, 0) X(256, 64, 2, 1, 0, 0) X(128, 64, 2, 0, 0, 0) X(128, 64, 2, 1, 0, 0) X(64, 64, 2, 0, 0, 0) X(64, 64, 2, 1, 0, 0) /* 1x1 */ \
    X(256, 64, 2, 1, 1, 1) X(128, 64, 2, 1, 1, 1) X(256, 64, 2, 1, 0, 1) X(128, 64, 2, 1, 0, 1)          /* 1x1 with the join (and sums) */ \
    X(256, 64, 1, 1, 1, 0) X(128, 64, 1, 1, 1, 0)                                                        /* input gradient with sums */ \
    X(256, 32, 1, 0, 0, 0) X(256, 64, 1, 1, 0, 0) X(128, 64, 1, 0, 0, 0) X(128, 64, 1, 1, 0, 0)          /* input gradient */
// dynamic LDS of the build with this key; -1: no such build
inline int convT_build_lds(long key) {
    switch (key) {
#define CONVT_LDS_CASE(BN, BK, MODE, BREG, BNS, JOIN) case convT_key(BN, BK, MODE, BREG, BNS, JOIN): return ConvTGeom<BN, BK, MODE, BREG, BNS, JOIN>::lds;
        CONVT_BUILDS(CONVT_LDS_CASE)
#undef CONVT_LDS_CASE
        default: return -1;
    }
}
enum ConvTKind { CONVT_NONE = 0, CONVT_FWD, CONVT_DGRAD, CONVT_1X1, CONVT_1X1_JOIN };
struct ConvTPlan {
    int kind;                   // CONVT_NONE: another kernel serves the launch, nothing below is meaningful
    int BN, BK, MODE;           // the build
    bool breg, bns, join;       //   bns: the launch forms BatchNorm-backward sums; join: the residual join in the epilogue
    bool bns_ok;                // an input gradient whose sums may ride along (register-fed builds, tiles inside one pass)
    bool join_ok;               // a 1x1 GEMM whose epilogue may take the join (and, with a.bny, the sums)
    int mt, nt, grid;           // 128-pixel tiles, column tiles, blocks
    int stat_rows;              // statistics rows written: one per 128-pixel tile
    int variant, lds;           // convT_variant of the build; its dynamic LDS bytes, -1 when there is no such build
    long key;                   // convT_key of the build
};

inline ConvTPlan convT_plan(const IgemmArgs& a, int flags) {
    ConvTPlan p = {};
    p.lds = -1;
    // what every kind needs: one 16-bit unit-stride source without pooling or offset, one 16-bit destination, 32-bit tile offsets
    if (a.nsrc != 1 || a.out_esz != 2 || a.out1) return p;
    const SrcDev& s = a.src[0];
    if (s.esz != 2 || s.sC != 1 || s.pool || s.off_y || s.off_x) return p;
    if (a.M >= (1l << 29) || a.Wb >= 32768) return p;
    const bool lds_w = (flags & CONVT_DBG_LDS_WEIGHTS) != 0;
    // the forward / 1x1 loaders address their source pixel-linearly: dense NHWC only (strided views take the generic kernel)
    const bool dense = s.C == a.Cin && s.sW == s.C && s.sH == (long)s.W * s.C && s.sN == (long)s.H * s.W * s.C;
    const bool same_extent = s.LH == a.Hb && s.LW == a.Wb;
    const long mt = cdiv(a.M, CONVT_BM);
    auto wide = [&](long blocks) { return a.Cout % 256 == 0 && mt * (a.Cout / 256) >= blocks; };     // the 256-column tile: enough blocks of it
    int BN = 0, BK = 64;
    if (a.nz == 4 && a.nseg == 1 && a.s_out == 2 && a.s_in == 1 && !a.stat) {
        // ConvTranspose forward as built by ustrun_convT2x2_fwd (4 parity classes, one segment); 128-pixel tiles must not straddle passes
        if (!same_extent || !dense || (s.gN > 0 && ((long)s.gN * a.Hb * a.Wb) % CONVT_BM)) return p;
        if (a.Cin % 64 || a.Cout % 64 || a.C0 != a.Cout) return p;
        p.kind = CONVT_FWD; p.MODE = 0; BN = 256; BK = lds_w ? 32 : 64;
    } else if (a.nz == 1 && a.nseg == 1 && a.s_out == 1 && a.s_in == 1 && a.d0 == 0) {
        // a 1x1 convolution at stride 1 (ustrun_conv2d_fwd, k = 1; ustrun_conv1x1_dgrad_join)
        if (!same_extent || !dense || s.gN > 0) return p;
        if (a.Cin % 64 || a.Cout % 64 || a.C0 != a.Cout || a.Ho != a.Hb || a.Wo != a.Wb) return p;
        // the join: a plain source, 128-column tiles, register-fed weights, 32-bit byte offsets behind a tile base
        p.join_ok = !lds_w && a.Cout % 128 == 0 && !a.bias && !s.scale && !s.relu && (long)a.M * a.Cout < (1L << 30);
        p.join = p.join_ok && (a.join_add || a.join_ref || a.bny);
        p.kind = p.join ? CONVT_1X1_JOIN : CONVT_1X1; p.MODE = 2;
        p.bns = p.join && a.bny;
        BN = wide(256) ? 256 : a.Cout % 128 == 0 ? 128 : 64;
        if (BN == 256 && lds_w) BK = 32;
    } else if (a.nz == 1 && a.nseg == 4 && a.segw == 2 && a.s_in == 2 && a.s_out == 1 && !(a.stat && !a.bny) && !a.bias) {
        // ConvTranspose input gradient as built by ustrun_convT2x2_dgrad (4 segments reading du at stride 2)
        if (s.scale || s.relu || s.H != 2 * a.Hb || s.W != 2 * a.Wb) return p;
        if (s.sW != s.C || s.sH != (long)s.W * s.C || s.sN != (long)s.H * s.W * s.C) return p;
        if (a.Cin % 64 || a.Cout % 128 || a.C0 != a.Cout) return p;
        // the sums: one statistics row per tile; the register-fed builds only, tiles inside one pass
        p.bns_ok = !lds_w && (a.bn_gN == 0 || ((long)a.bn_gN * a.Hb * a.Wb) % CONVT_BM == 0);
        p.bns = a.bny && p.bns_ok;
        p.kind = CONVT_DGRAD; p.MODE = 1;
        BN = wide(512) ? 256 : 128;
        if (BN == 256 && lds_w && !p.bns) BK = 32;
    } else return p;
    p.BN = BN; p.BK = BK;
    p.breg = p.bns || p.join || !lds_w;
    p.mt = (int)mt; p.nt = (p.MODE == 0 ? 4 * a.Cout : a.Cout) / BN; p.grid = p.mt * p.nt;
    p.stat_rows = p.mt;
    p.variant = convT_variant(BN, BK, p.MODE, p.breg, p.bns, p.join);
    p.key = convT_key(BN, BK, p.MODE, p.breg, p.bns, p.join);
    p.lds = convT_build_lds(p.key);
    return p;
}

// ---- the weight gradient.  Round-1 kernel: 128 ci x (4 taps x 32 co) per block, 64-pixel stages, two buffers.  Round-5 kernel (T2): TM ci x
// (4 taps x 64 co), 32-pixel stages, three stage buffers ----
constexpr int WGT_TM = 128, WGT_KP = 64, WGT_RB = 256, WGT_LDS = 4 * WGT_KP * WGT_RB;      // round 1: ci tile, pixels per stage, LDS row pitch, LDS bytes
constexpr int KP2 = 32, BRB2 = 512;                          // round 5: pixels per stage, du row pitch
template <int TM> struct T2 {
    static constexpr int ARB = TM * 2;                       // activation row pitch (bytes)
    static constexpr int ATILE = KP2 * ARB, BTILE = KP2 * BRB2, STAGE = ATILE + BTILE;
    static constexpr int NTH = 2 * TM;                       // threads: 512 / 256
    static constexpr int AIT = KP2 * (TM / 8) / NTH;         // 16-byte activation items per thread and stage: 2
    static constexpr int BIT = KP2 * 32 / NTH;               // du items: 2 / 4
    static constexpr int WM = TM / 64, WN = 2;               // waves along ci / along the columns (one 32-co half each)
    static constexpr int NT = 4, lds = 3 * STAGE;            // du fragments (8 co x 4 taps each) per wave; three stage buffers
};
// the builds: R1() the round-1 kernel, T(TM, DIAG) the round-5 kernel.  The DIAG build (phase stamps) is no plan's choice: the launch
// takes it in place of T(256, 0) while ustrun_debug_buffer is set.
#define WGRADT_BUILDS(R1, T) R1() T(256, 1) T(256, 0) T(128, 0)

struct WgradTPlan {
    bool ok;                    // one of the two kernels serves the launch
    int kernel;                 // 1: the round-1 kernel, 2: the round-5 kernel
    int tm, cols;               // ci per block, co per column tile (x 4 taps)
    int stage, threads;         // pixels per stage, threads per block
    int ksplit; long kchunk;    // split-K over the pixels: slabs, pixels per slab (whole stages)
    int grid, lds, variant;
};
inline bool wgradT_base_ok(const WgradArgs& a) {
    if (a.nseg != 4 || a.segw != 2 || a.dy_s != 2 || a.astep != 0 || a.d0 != 0 || a.ashift != 0 || a.dy_esz != 2 || a.nsrc != 1) return false;
    const SrcDev& s = a.src[0];
    if (s.esz != 2 || s.sC != 1 || s.pool || s.off_y || s.off_x || s.LH != a.Hb || s.LW != a.Wb) return false;
    if ((s.relu && !s.scale) || (s.sW & 7)) return false;
    if (s.sH != (long)a.Wb * s.sW || s.sN != (long)a.Hb * s.sH) return false;      // pixel-linear source
    if (a.dyH != 2 * a.Hb || a.dyW != 2 * a.Wb || a.Wb >= 32768) return false;
    return true;
}
// split-K over the M pixels, parameterised by the blocks of one resident round, the pixels per stage and the least stages per block
inline int wgradT_splitk(long tiles, int resident, int kp, int min_stages, long M, long* kchunk) {
    long ks = (resident + tiles - 1) / tiles;
    if (ks > M / (min_stages * kp)) ks = M / (min_stages * kp);
    if (ks < 1) ks = 1;
    *kchunk = ((M + ks - 1) / ks + kp - 1) / kp * kp;
    return (int)((M + *kchunk - 1) / *kchunk);
}
// ... of round 1: 2 blocks per CU, four 64-pixel stages; of round 5 (Cin alone decides the tile): one 256-ci block or two 128-ci blocks per
// CU, eight 32-pixel stages
inline int wgradT_ksplit(int kernel, int Cin, int Cout, long M, long* kchunk) {
    const int tm = Cin % 256 == 0 ? 256 : 128;
    return kernel == 1 ? wgradT_splitk((long)(Cin / WGT_TM) * (Cout / 32), 512, WGT_KP, 4, M, kchunk)
                       : wgradT_splitk((long)(Cin / tm) * (Cout / 64), tm == 256 ? 256 : 512, KP2, 8, M, kchunk);
}
// the largest ksplit either kernel can choose for (Cin, Cout, npix): what ustrun_wgrad_partials_bytes publishes; 0: neither runs
inline int wgradT_max_ksplit(int Cin, int Cout, long npix) {
    long chunk;
    if (Cin % 128 || Cout % 32) return 0;
    const int k1 = wgradT_ksplit(1, Cin, Cout, npix, &chunk), k2 = Cout % 64 == 0 ? wgradT_ksplit(2, Cin, Cout, npix, &chunk) : 0;
    return k1 > k2 ? k1 : k2;
}

inline WgradTPlan wgradT_plan(const WgradArgs& a, int flags) {
    WgradTPlan p = {};
    if (!wgradT_base_ok(a)) return p;
    const SrcDev& s = a.src[0];
    const long gpix = s.gN > 0 ? (long)s.gN * a.Hb * a.Wb : 0;      // stages must not straddle passes
    // the round-5 kernel: whole 64-co column tiles, 128 / 256-ci row tiles, rows of >= 16 pixels (a 32-pixel stage wraps at most two
    // image rows), 32-bit item offsets
    const bool t2 = !(flags & WGRADT_DBG_ROUND1) && a.Cout % 64 == 0 && a.Cin % 128 == 0 && a.Wb >= 16 && gpix % KP2 == 0 &&
                    (long)KP2 * s.sW * 2 + (long)a.Cin * 2 < (1L << 30) && (2L * KP2 + 6L * a.Wb + 2) * a.Cout * 2 < (1L << 30);
    if (t2) {
        p.kernel = 2; p.tm = a.Cin % 256 == 0 ? 256 : 128; p.cols = 64; p.stage = KP2; p.threads = 2 * p.tm;
        p.lds = p.tm == 256 ? T2<256>::lds : T2<128>::lds; p.variant = 0x54320000 | p.tm;      // 'T2' | ci tile
    } else {
        if (gpix % WGT_KP || a.Cin % 128 || a.Cout % 32) return p;
        p.kernel = 1; p.tm = WGT_TM; p.cols = 32; p.stage = WGT_KP; p.threads = 256;
        p.lds = WGT_LDS; p.variant = 0x54310000;                                               // 'T1'
    }
    p.ok = true;
    p.ksplit = wgradT_ksplit(p.kernel, a.Cin, a.Cout, a.M, &p.kchunk);
    p.grid = (a.Cin / p.tm) * (a.Cout / p.cols) * p.ksplit;
    return p;
}

}  // namespace ustrun
