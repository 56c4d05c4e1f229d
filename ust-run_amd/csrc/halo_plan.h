// halo_plan.h -- the tile plan of the 3x3 halo convolution (conv_halo_bf16.hip): the geometry of a build (HaloGeom: patch, staging and
// dynamic LDS, read by the kernel and by its launch), the list of builds (HALO_BUILDS: what the dispatch instantiates), and the ONE
// decision "which build serves this launch, and what follows from it" (halo_plan: tile counts, statistics rows, BatchNorm-backward sum
// eligibility, pass sizes of the linear tiles, the variant code the tests read).  Pure host integer code without device-only
// constructs: tests/host/halo_plan_check.hip compiles it for the host and pins it over a sweep of shapes and debug flags.
#pragma once
#include "common.h"

namespace ustrun {

// ---- the bits of ustrun_debug_flags / ustrun_debug_flags2 this plan reads (A/B runs and the tests that pin the flag-only builds) ----
constexpr int HALO_DBG_LDS_WEIGHTS = 8;             // bit 3: weights through LDS (register-fed weights off)
constexpr int HALO_DBG_FORCE_SHIFT = 10, HALO_DBG_FORCE_MASK = 3;   // bits 10-11: force 128-column tile 0..2 (value - 1)
constexpr int HALO_DBG_TILE512 = 8192;              // bit 13: the 512-pixel x 64-channel tile
constexpr int HALO_DBG_M16_ALL = 32768;             // bit 15: every plain-source tile on the 16x16x32 build
constexpr int HALO_DBG_M16_NONE = 2097152;          // bit 21: no tile on the 16x16x32 build
constexpr int HALO_DBG2_NO_LINEAR = 1;              // flags2 bit 0: no linear tiles

// ---- geometry of one build, over the kernel's template parameters ----
template <int TH, int TW, int BN, int BK, int MI, bool POOL, int NT, bool XF, int DIL = 1, bool BREG = false, bool M16 = false, bool BNS = false,
          int LINW = 0>
struct HaloGeom {
    static_assert(BK == 32, "80-byte patch rows hold one 32-channel chunk");
    static constexpr bool LIN = LINW > 0;
    static constexpr int RP = LINW + 1, TM = TH * TW;  // RP: row pitch of the flat padded space (LIN)
    static_assert(!LIN || (DIL == 1 && !POOL && TW == 32 && BREG && RP > 8), "linear tiles: un-dilated, un-pooled, 32-position sub-tiles");
    static_assert(!M16 || (BREG && !XF), "the 16x16x32 build: plain sources, weights through registers");
    static_assert(!BNS || M16, "BatchNorm-backward sums ride on the 16x16x32 epilogue (8 channels of a pixel per lane)");
    static_assert(!BREG || NT <= 2, "register-fed weights: 16 registers per tap and set");
    static constexpr int HW2 = LIN ? RP : TW + 2 * DIL;
    static constexpr int SR = 32 / TW;                 // tile rows per 32-pixel sub-tile (2 or 1)
    static constexpr int WM = TH / (SR * MI), WN = 4 / WM;
    static_assert(WM * WN == 4 && BN == WN * 64, "4 waves, 64 channels per wave");
    static constexpr int HP = LIN ? TM + 2 * RP + 2 : (TH + 2 * DIL) * HW2;    // halo pixels
    static constexpr int PITCH = 80;                   // patch row: 4 x 16 B of channels + 16 B pad
    static constexpr int DSLOTS = (HP * 5 + 63) / 64 * 64;   // direct staging: 16-byte LDS slots incl. the pad slots, whole waves
    static constexpr int XSLOTS = (HP * 4 + 63) / 64 * 64;   // transform staging: (pixel, channel group) items, whole waves
    static constexpr int AIT = (DSLOTS + 255) / 256;   // staging steps per chunk (taps 0 .. AIT-1), one item per thread each
    static constexpr int NSTG = (9 + NT - 1) / NT;     // stages per chunk: NT taps (weight tiles) per barrier
    static constexpr int BATCH = (AIT + NSTG - 2) / (NSTG - 1);   // patch items per stage; the chunk's last stage carries the constants
    static_assert(BATCH * (NSTG - 1) >= AIT, "staging fits the chunk");
    static constexpr int NP = POOL ? 4 : 1;
    // BREG: every wave issues every staging step (its transfer counts are then compile-time constants, see the counted wait):
    // the slots past the patch image are a few hundred bytes of trash behind it
    static constexpr int ABYTES = (BREG ? AIT * 256 : DSLOTS) * 16;
    static constexpr int BCH = (BK / 8) * BN, BIT = BCH / 256;     // 16-byte chunks per B tile
    static_assert(BCH % 256 == 0, "B tile must be a whole number of wave-instructions per wave");
    static constexpr int RAWB = XF ? BATCH * NP * 4096 : 0;   // a raw slot: BATCH x NP x 16 B per thread
    static constexpr int BBYTES = BREG ? 0 : 2 * NT * BCH * 16;
    // SKEW: the items a stage fetches are transformed under the NEXT stage's MFMAs (two raw slots, by stage parity) --
    // where a second slot still leaves room for two blocks per CU; otherwise after the stage's own MFMAs
    static constexpr bool SKEW = XF && 2 * ABYTES + BBYTES + 2 * RAWB + 512 <= 81920;
    // dynamic LDS: 2 x patch, 2 x NT weight tiles (none with BREG), NRAW raw slots, 2 x {32 scales, 32 shifts} f32
    static constexpr int NRAW = SKEW ? 2 : 1;
    static constexpr int lds = 2 * ABYTES + BBYTES + NRAW * RAWB + 512;
};

// ---- the builds: X(TH, TW, BN, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW).  A tile comes as four 32x32x16 builds -- weights through
// registers / LDS x transforming / plain source (HALO_QUAD) --, un-dilated tiles also as a 16x16x32 build for plain sources with
// register-fed weights (HALO_M16 = that build + the four), and where sums are formed as a 16x16x32 build with the BatchNorm-backward
// sums in the epilogue (HALO_BNS); a linear tile of row length W with sums, transforming, and 16x16x32 plain (HALO_LIN).  The
// transforming variants are not built on 16x16x32 (160 registers past the file), the pooled tile only with weights through LDS.
// U rows: kernels the code object has always carried although no plan selects them (each rate's 128-column tile at the other rate).
// The kernels lie in the code object in the order of this list. ----
#define HALO_QUAD(X, TH, TW, BN, MI, NT, DIL) \
    X(TH, TW, BN, MI, 0, NT, 1, DIL, 1, 0, 0, 0) X(TH, TW, BN, MI, 0, NT, 0, DIL, 1, 0, 0, 0) \
    X(TH, TW, BN, MI, 0, NT, 1, DIL, 0, 0, 0, 0) X(TH, TW, BN, MI, 0, NT, 0, DIL, 0, 0, 0, 0)
#define HALO_M16(X, TH, TW, BN, MI, NT, DIL) X(TH, TW, BN, MI, 0, NT, 0, DIL, 1, 1, 0, 0) HALO_QUAD(X, TH, TW, BN, MI, NT, DIL)
#define HALO_BNS(X, TH, TW, BN, MI, NT, DIL) X(TH, TW, BN, MI, 0, NT, 0, DIL, 1, 1, 1, 0)
#define HALO_LIN(X, W) X(8, 32, 128, 4, 0, 1, 0, 1, 1, 1, 1, W) X(8, 32, 128, 4, 0, 1, 1, 1, 1, 0, 0, W) X(8, 32, 128, 4, 0, 1, 0, 1, 1, 1, 0, W)
#define HALO_BUILDS(X, U) \
    HALO_BNS(U, 16, 16, 128, 4, 1, 2) HALO_BNS(X, 8, 16, 128, 2, 2, 2)                                       /* dilation 2 */ \
    HALO_QUAD(U, 16, 16, 128, 4, 1, 2) HALO_QUAD(X, 8, 16, 128, 2, 2, 2) HALO_QUAD(X, 8, 16, 64, 1, 2, 2) \
    HALO_BNS(X, 16, 16, 128, 4, 1, 4) HALO_BNS(U, 8, 16, 128, 2, 2, 4)                                       /* dilation 4 */ \
    HALO_QUAD(X, 16, 16, 128, 4, 1, 4) HALO_QUAD(U, 8, 16, 128, 2, 2, 4) HALO_QUAD(X, 8, 16, 64, 1, 2, 4) \
    HALO_LIN(X, 18) HALO_LIN(X, 24) HALO_LIN(X, 36) HALO_LIN(X, 72) \
    X(8, 16, 128, 2, 1, 2, 1, 1, 0, 0, 0, 0)                                                                 /* pooled source */ \
    HALO_BNS(X, 8, 32, 128, 4, 1, 1) HALO_M16(X, 8, 32, 128, 4, 1, 1)                                        /* 128 columns: tile 0 */ \
    HALO_BNS(X, 16, 16, 128, 4, 1, 1) HALO_M16(X, 16, 16, 128, 4, 1, 1)                                      /* tile 1 */ \
    HALO_M16(X, 8, 16, 64, 1, 2, 1) HALO_M16(X, 8, 16, 128, 2, 2, 1)                                         /* tile 3 (small grids), tile 2 */ \
    HALO_M16(X, 16, 32, 64, 4, 1, 1) HALO_M16(X, 8, 32, 64, 2, 2, 1) HALO_M16(X, 16, 16, 64, 2, 2, 1)        /* 64 columns: 512 pixels, wide, narrow */
#define HALO_NONE(...)

// the code ustrun_debug_last_conv_variant reports: TH<<24 | TW<<16 | BN<<8 | M16<<7 | MI<<4 | NT<<2 | POOL<<1 | XF (linear tiles:
// bit 30 | W<<16 | ...)
constexpr int halo_variant(int TH, int TW, int BN, int MI, bool POOL, int NT, bool XF, bool M16, int LINW) {
    return (LINW ? (1 << 30 | LINW << 16) : (TH << 24 | TW << 16)) | BN << 8 | (M16 ? 0x80 : 0) | MI << 4 | NT << 2 | (POOL ? 2 : 0) | (XF ? 1 : 0);
}
// a build's key: the variant code and, above it, what the code leaves out
constexpr long halo_key(int TH, int TW, int BN, int MI, bool POOL, int NT, bool XF, int DIL, bool BREG, bool M16, bool BNS, int LINW) {
    return (long)(DIL | (BREG ? 8 : 0) | (BNS ? 16 : 0)) << 32 | halo_variant(TH, TW, BN, MI, POOL, NT, XF, M16, LINW);
}
// dynamic LDS of the build with this key; -1: no such build
inline int halo_build_lds(long key) {
    switch (key) {
#define HALO_LDS_CASE(TH, TW, BN, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW) \
    case halo_key(TH, TW, BN, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW): return HaloGeom<TH, TW, BN, 32, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW>::lds;
        HALO_BUILDS(HALO_LDS_CASE, HALO_NONE)
#undef HALO_LDS_CASE
        default: return -1;
    }
}

// can this conv3x3-shaped problem run on the halo kernel?
inline bool halo_plan_supported(const IgemmArgs& a) {
    if (a.nseg != 9 || a.nz != 1 || a.s_in != 1 || a.s_out != 1 || a.segw != 3) return false;
    const int dil = a.dstep < 0 ? -a.dstep : a.dstep;
    if (a.d0 != -a.dstep || !(dil == 1 || dil == 2 || dil == 4)) return false;      // (other rates: the generic kernel)
    if (a.out_esz != 2 || (a.C0 & 7) || ((a.Cout - a.C0) & 7) || a.bias) return false;     // (3x3 convs here carry no bias)
    bool pool = false;
    for (int i = 0; i < a.nsrc; ++i) {
        if (a.src[i].sC != 1 || (a.src[i].C & 7) || a.src[i].esz != 2) return false;
        pool |= a.src[i].pool != 0;
    }
    if (a.Cin % 32 || a.Cout % 64 || (a.nsrc == 2 && (a.src[0].C % 32))) return false;      // whole 32-channel chunks per source
    if (pool && (a.nsrc != 1 || a.Cout % 128)) return false;
    if (a.Hb < 4 || a.Wb < 8) return false;      // tiny extents: the generic kernel wastes less
    if (dil > 1 && (pool || a.nsrc != 1)) return false;
    return true;
}

struct HaloPlan {
    bool ok;                    // halo_plan_supported: everything below is meaningful
    int TH, TW, BN, MI, NT;     // the build
    bool pool, xf;              //   xf: some source needs arithmetic on load (BatchNorm affine, ReLU, pooling)
    bool breg, m16, bns;        //   bns: the launch forms BatchNorm-backward sums (a.bny is set and bns_ok)
    int dil, linw;              //   linw: the row length of linear tiles, else 0
    bool bns_ok;                // an eligible plain-source input gradient whose build has a sums instantiation
    int tiles_x, tiles_y;       // tiles per image row / column (linear: tiles per full pass / images per pass = the pass size)
    int mtiles, ntiles;         // M tiles of the launch, column tiles
    int stat_rows;              // statistics rows written: one per 8 tile rows of an M tile (linear: one per tile)
    int last_rows;              // linear: statistics rows of the last pass (-1: not linear, or a single pass)
    int variant, lds;           // halo_variant of the build; its dynamic LDS bytes, -1 when there is no such build
    long key;                   // halo_key of the build
};

// The tiles' measured relative rates on full tiles (8 x 32: 1, 16 x 16: 0.93, 8 x 16 with two sub-tiles per wave: 0.80 --
// profiles/r03_ab_halo_tiles.log: 512 -> 512 at 48 x 48: 0.346 -> 0.290 ms on 16 x 16 tiles; 1024 -> 1024 at 18 x 18 and 24 x 24: -9 %
// on 8 x 16) and the padded area of a map on each: rate x useful MFMA fraction is what tile choice and linear tiles compare.
constexpr double HALO_RATE[3] = {1.0, 0.93, 0.80};
inline double halo_pad_area(const IgemmArgs& a, int t) {      // tile t = 0 (8 x 32), 1 (16 x 16), 2 (8 x 16)
    return (cdiv(a.Hb, t == 1 ? 16 : 8) * (t == 1 ? 16.0 : 8.0)) * (cdiv(a.Wb, t ? 16 : 32) * (t ? 16.0 : 32.0));
}

// Tile of the 128-column, un-pooled, un-dilated case: 0 = 8 x 32 px (MI 4), 1 = 16 x 16 px (MI 4), 2 = 8 x 16 px (MI 2, 128 columns),
// 3 = 8 x 16 px, 64 columns (less than one block per CU).  HALO_DBG_FORCE forces 0..2 (+1) for A/B runs.
inline int halo_tile128(const IgemmArgs& a, int flags) {
    const int force = (flags >> HALO_DBG_FORCE_SHIFT) & HALO_DBG_FORCE_MASK;
    const bool wide = a.Wb >= 32;                 // 32-pixel rows: conflict-free A fragment reads
    if (force) return (force == 1 && !wide) ? 1 : force - 1;
    // 16-row tiles (256 px x 128 ch per block) read fewer LDS/weight bytes per flop but need >= 2 blocks per CU
    if ((long)a.N * cdiv(a.Hb, 16) * cdiv(a.Wb, 16) * (a.Cout / 128) >= 512) {
        // enough blocks for any tile: the one that wastes the fewest MFMAs on padding, weighted by the rates.  Maps whose sides are
        // multiples of 32 (every level of the 256 x 256 workloads) keep the 8 x 32 tile.
        const double s0 = wide ? HALO_RATE[0] / halo_pad_area(a, 0) : 0.0, s1 = HALO_RATE[1] / halo_pad_area(a, 1), s2 = HALO_RATE[2] / halo_pad_area(a, 2);
        return (s0 >= s1 && s0 >= s2) ? 0 : (s1 >= s2 ? 1 : 2);
    }
    if ((long)a.N * cdiv(a.Hb, 8) * cdiv(a.Wb, 16) * (a.Cout / 128) < 256) return 3;      // less than one block per CU
    return 2;
}

inline HaloPlan halo_plan(const IgemmArgs& a, int flags, int flags2) {
    HaloPlan p = {};
    p.last_rows = p.lds = -1;
    if (!(p.ok = halo_plan_supported(a))) return p;
    p.dil = a.dstep < 0 ? -a.dstep : a.dstep;
    for (int i = 0; i < a.nsrc; ++i) {
        p.pool |= a.src[i].pool != 0;
        p.xf |= a.src[i].pool != 0 || a.src[i].scale != nullptr || a.src[i].relu != 0;
    }
    const bool c128 = a.Cout % 128 == 0, wide = a.Wb >= 32;
    const bool force = ((flags >> HALO_DBG_FORCE_SHIFT) & HALO_DBG_FORCE_MASK) != 0;
    const bool m16_off = (flags & (HALO_DBG_LDS_WEIGHTS | HALO_DBG_M16_NONE)) != 0;
    p.breg = !p.pool && !(flags & HALO_DBG_LDS_WEIGHTS);       // weights through registers, one barrier per chunk
    const int t128 = halo_tile128(a, flags);
    // Linear tiles (18, 24, 36, 72-pixel rows) serve 128-column outputs of un-pooled, un-dilated sources when (a) the rectangular tile
    // would waste more of its MFMAs on padding -- useful fraction x rate -- and (b) the launch still has a block per CU.  A pass =
    // the images that share BatchNorm constants (the call's pass_gN, the sources' gN, or the gN of the BatchNorm-backward sums the
    // launch forms; the whole batch without any): tiles never cross one, so sizes that disagree keep the rectangular tiles.
    if (const int w = a.Wo; !(flags2 & HALO_DBG2_NO_LINEAR) && !(flags & HALO_DBG_M16_ALL) && !m16_off && !force && p.dil == 1 && !p.pool && c128 && a.Hb == a.Ho &&
        a.Wb == a.Wo && (w == 18 || w == 24 || w == 36 || w == 72)) {
        int g = a.pass_gN > 0 ? a.pass_gN : 0, clash = 0;
        for (int i = 0; i < a.nsrc; ++i)
            if (a.src[i].gN > 0) { clash |= g && g != a.src[i].gN; g = a.src[i].gN; }
        if (a.bn_gN > 0) { clash |= a.bny && g && g != a.bn_gN; if (!g) g = a.bn_gN; }
        if (g <= 0 || g > a.N) g = a.N;
        for (int i = 0; i < a.nsrc; ++i) clash |= (long)g * a.src[i].sN * 2 >= (1L << 31) - 4096;      // 32-bit byte offsets inside a pass
        const long IS = (long)(a.Ho + 1) * (a.Wo + 1);         // positions per image of the flat padded space
        const int tpp = cdiv(g * IS, 256), full = a.N / g, tailN = a.N - full * g, tail = cdiv(tailN * IS, 256), mtiles = full * tpp + tail;
        const double lin = (double)a.N * a.Ho * a.Wo / (mtiles * 256.0);
        const int tr = t128 > 2 ? 2 : t128;                    // (tile 3 is tile 2's pixels)
        if (!clash && (long)mtiles * (a.Cout / 128) >= 160 && lin > 1.05 * (HALO_RATE[tr] * ((double)a.Hb * a.Wb) / halo_pad_area(a, tr))) {
            p.linw = w; p.tiles_x = tpp; p.tiles_y = g; p.mtiles = mtiles;
            p.last_rows = tailN ? tail : (full > 1 ? tpp : -1);
        }
    }

    auto tile = [&p](int TH, int TW, int BN, int MI, int NT) { p.TH = TH; p.TW = TW; p.BN = BN; p.MI = MI; p.NT = NT; };
    // MI = 2 tiles run two taps per barrier (16 MFMAs per wave and stage, like the MI = 4 tiles)
    if (p.dil > 1) {
        // dilated 3x3 (DeepLabV2-ResNet layer3 / layer4): 8 x 16-pixel tiles keep the (8 + 2d) x (16 + 2d) patch pair small at rate 2
        // (two blocks per CU; the large tile measured 0.089 -> 0.108 ms there).  Rate 4: the 16 x 24 patch of an 8 x 16 tile is three times
        // its output and its pair of buffers leaves room for ONE block per CU anyway -- a 16 x 16 tile (24 x 24 patch: 2.25 x) with the 4 x 2
        // wave tile does twice the MFMA work per stage in that one block: 0.49 -> 0.39 ms on layer4's 512 -> 512 convolutions
        if (!c128) tile(8, 16, 64, 1, 2);
        else if (p.dil == 4) tile(16, 16, 128, 4, 1);
        else tile(8, 16, 128, 2, 2);
    } else if (p.pool) tile(8, 16, 128, 2, 2);
    else if (p.linw) tile(8, 32, 128, 4, 1);
    else if (c128) {
        // 256 px x 128 ch per block, wave tile 128 px x 64 ch (tiles 0, 1); less than one block per CU (the batch-1 forward,
        // validation at test_bs 1): twice the blocks at 64 channels each (tile 3: 20-25 % faster per layer at batch 1)
        switch (t128) {
            case 0: tile(8, 32, 128, 4, 1); break;
            case 1: tile(16, 16, 128, 4, 1); break;
            case 3: tile(8, 16, 64, 1, 2); break;
            default: tile(8, 16, 128, 2, 2); break;
        }
    } else if (wide && (flags & HALO_DBG_TILE512) && a.Hb >= 16) tile(16, 32, 64, 4, 1);      // wave tile 128 px x 64 ch, one block per CU -- A/B runs
    else if (wide) tile(8, 32, 64, 2, 2);
    else tile(16, 16, 64, 2, 2);

    // BatchNorm-backward sums (the input gradient that produces da of a BatchNorm + ReLU layer): one plain source, one destination,
    // the two 256-pixel x 128-channel tiles, the linear tiles and the dilated 128-column tiles -- always on the 16x16x32 build
    p.bns_ok = a.nsrc == 1 && !a.out1 && a.C0 == a.Cout && c128 && !p.xf && !m16_off &&
               (p.dil != 1 ? a.bn_gN == 0 : (p.MI == 4 && p.NT == 1 && p.BN == 128));
    p.bns = a.bny && p.bns_ok;
    // the 16x16x32 build (measured ahead on the input gradients of every layer, profiles/r04_ab_halo_m16.log: 512 -> 512 at 32 x 32
    // 0.220 -> 0.202 ms, 1024 -> 1024 0.217 -> 0.201, 128 -> 128 -1.5 %): the default for plain sources on the 256-pixel tiles
    p.m16 = p.bns || (p.dil == 1 && !p.xf && !m16_off && ((flags & HALO_DBG_M16_ALL) || (p.MI == 4 && p.NT == 1)));

    if (!p.linw) { p.tiles_x = cdiv(a.Wb, p.TW); p.tiles_y = cdiv(a.Hb, p.TH); p.mtiles = a.N * p.tiles_y * p.tiles_x; }
    p.ntiles = a.Cout / p.BN;
    p.stat_rows = p.linw ? p.mtiles : p.mtiles * (p.TH / 8);
    p.variant = halo_variant(p.TH, p.TW, p.BN, p.MI, p.pool, p.NT, p.xf, p.m16, p.linw);
    p.key = halo_key(p.TH, p.TW, p.BN, p.MI, p.pool, p.NT, p.xf, p.dil, p.breg, p.m16, p.bns, p.linw);
    p.lds = halo_build_lds(p.key);
    return p;
}

}  // namespace ustrun
