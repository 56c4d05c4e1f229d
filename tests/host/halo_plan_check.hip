// halo_plan_check.hip -- host-only check of the tile plan of the 3x3 halo convolution (ust-run_amd/csrc/halo_plan.h) over a sweep of
// shapes, sources and debug flags (tests/test_halo_plan_host.py builds and runs it; no GPU, no device code is called).  Exit status 0 =
// every check passed.  Arguments:
//   rows                                       also print, for every swept launch ustrun_debug_conv_stat_rows can express (one dense source,
//                                              plain or pooled, one pass), "rows N H W Cin Cout dilation pooled flags flags2 stat_rows"
//   pin=N,c0,c1,Cout,H,W,G,plain,f1,f2,vf,vd   the forward (sources of c0 [+ c1] channels, G passes) and the input gradient of one layer
//                                              must plan the variant codes vf / vd under flags f1 / f2
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "../../ust-run_amd/csrc/halo_plan.h"

using namespace ustrun;

static long g_fail = 0;
struct Spec { int N, H, W, c0, c1, Cout, dil, kind, gN, bny, dgrad; };      // kind: 0 plain, 1 transforming, 2 pooled first source
static void fail(const char* what, const Spec& s, int f1, int f2, long a, long b) {
    if (g_fail++ < 20)
        std::printf("FAIL %s (N = %d, %d x %d, %d + %d -> %d, dilation %d, kind %d, gN %d, bny %d, flags %d / %d): %ld, %ld\n", what, s.N, s.H, s.W,
                    s.c0, s.c1, s.Cout, s.dil, s.kind, s.gN, s.bny, f1, f2, a, b);
}

static SrcDev src(int C, int H, int W, int kind, int gN, int oy, int ox) {
    ustrun_src_t d = {};
    const int m = kind == 2 ? 2 : 1;
    d.ptr = (const void*)16; d.C = C; d.H = m * H; d.W = m * W;
    d.sC = 1; d.sW = C; d.sH = (int64_t)d.W * C; d.sN = (int64_t)d.H * d.sH;
    d.pool = kind == 2; d.relu = kind != 0;
    if (kind == 1) d.scale = d.shift = (const float*)16;
    d.gN = gN; d.gstride = 4 * C; d.off_y = oy; d.off_x = ox;
    return make_src(d, USTRUN_D16);
}

// the launch as ops.hip / resnet_ops.hip describe it: forward (a second source is a plain tensor of smaller extent at an offset), or
// the input gradient (one plain source, taps walked backwards), optionally forming BatchNorm-backward sums
static IgemmArgs make_args(const Spec& s) {
    IgemmArgs a = {};
    a.nsrc = s.c1 ? 2 : 1;
    a.src[0] = src(s.c0, s.H, s.W, s.kind, s.gN, 0, 0);
    if (s.c1) a.src[1] = src(s.c1, s.H - 2, s.W - 4, 0, 0, 1, 2);
    a.Cin = s.c0 + s.c1; a.W = (const float*)16; a.Cout = s.Cout;
    a.N = s.N; a.Hb = s.H; a.Wb = s.W; a.M = s.N * s.H * s.W;
    a.s_in = 1; a.nseg = 9; a.segw = 3; a.d0 = s.dgrad ? s.dil : -s.dil; a.dstep = -a.d0;
    a.nz = 1; a.s_out = 1;
    a.out0 = (float*)16; a.C0 = s.Cout; a.Ho = s.H; a.Wo = s.W; a.out_esz = 2;
    a.stat = (float*)16; a.pass_gN = s.gN;
    if (s.bny) { a.bny = (const void*)16; a.bnsc = a.bnsh = (const float*)16; a.bn_gN = s.gN; a.bn_gstride = 4 * s.Cout; }
    return a;
}

// the one list of builds, as the dispatch has it: key, HaloGeom's LDS bytes, and how often the sweep reached each
struct Build { long key; int lds; const char* name; long hits; };
#define ROW(TH, TW, BN, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW) \
    {halo_key(TH, TW, BN, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW), HaloGeom<TH, TW, BN, 32, MI, POOL, NT, XF, DIL, BREG, M16, BNS, LINW>::lds, \
     #TH "x" #TW "x" #BN " MI" #MI " pool" #POOL " NT" #NT " xf" #XF " dil" #DIL " breg" #BREG " m16" #M16 " bns" #BNS " lin" #LINW, 0},
static Build g_builds[] = {HALO_BUILDS(ROW, HALO_NONE)};
#undef ROW
static const int NBUILD = sizeof(g_builds) / sizeof(g_builds[0]);

static int published_bound(int N, int H, int W, int Cout) {       // ustrun_conv_mtiles (ops.hip)
    const int lin = cdiv((int64_t)N * H * W, 128), tiled = N * cdiv(H, 16) * 2 * cdiv(W, 16), stream = Cout == 64 ? 2 * N * cdiv(W, 32) * cdiv(H, 8) : 0;
    const int m = lin > tiled ? lin : tiled;
    return m > stream ? m : stream;
}

// every property one plan must have; returns false when the halo kernel does not take the launch
static bool check_plan(const Spec& s, int f1, int f2, HaloPlan* out = nullptr) {
    const IgemmArgs a = make_args(s);
    const HaloPlan p = halo_plan(a, f1, f2);
    if (out) *out = p;
    if (p.ok != halo_plan_supported(a)) fail("ok", s, f1, f2, p.ok, 0);
    if (!p.ok) return false;
    // the build exists, with HaloGeom's LDS size, inside the 160 KB of a CU
    int b = 0;
    while (b < NBUILD && g_builds[b].key != p.key) ++b;
    if (b == NBUILD) { fail("the plan names no build of the dispatch", s, f1, f2, p.variant, p.key >> 32); return true; }
    ++g_builds[b].hits;
    if (p.lds != g_builds[b].lds || p.lds <= 0 || p.lds > 160 * 1024) fail("LDS bytes", s, f1, f2, p.lds, g_builds[b].lds);
    if (p.key != halo_key(p.TH, p.TW, p.BN, p.MI, p.pool, p.NT, p.xf, p.dil, p.breg, p.m16, p.bns, p.linw)) fail("key", s, f1, f2, p.key, 0);
    if (p.variant != (int)(p.key & 0xffffffffL)) fail("variant", s, f1, f2, p.variant, p.key);
    // tiles and statistics rows
    if (p.ntiles * p.BN != a.Cout) fail("column tiles", s, f1, f2, p.ntiles, p.BN);
    if (p.linw) {
        if (p.pool || p.dil != 1 || p.BN != 128 || p.linw != s.W || p.TH * p.TW != 256 || !p.breg) fail("linear tiles: un-pooled, un-dilated, 128 columns", s, f1, f2, p.linw, p.BN);
        const long IS = (long)(s.H + 1) * (s.W + 1);
        const int g = p.tiles_y;
        long tiles = 0, last = 0, passes = 0;
        for (int n0 = 0; n0 < s.N; n0 += g, ++passes) tiles += last = cdiv((s.N - n0 < g ? s.N - n0 : g) * IS, 256);
        if (g < 1 || g > s.N || (s.gN && g != s.gN) || p.tiles_x != cdiv(g * IS, 256) || p.mtiles != tiles) fail("linear tiles: passes", s, f1, f2, p.mtiles, tiles);
        if (p.stat_rows != p.mtiles) fail("linear tiles: one statistics row per tile", s, f1, f2, p.stat_rows, p.mtiles);
        if (p.last_rows != (passes > 1 ? last : -1)) fail("linear tiles: rows of the last pass", s, f1, f2, p.last_rows, last);
    } else {
        if (p.tiles_x != cdiv(s.W, p.TW) || p.tiles_y != cdiv(s.H, p.TH) || p.mtiles != s.N * p.tiles_x * p.tiles_y) fail("tiles", s, f1, f2, p.mtiles, p.tiles_x);
        if (p.TH % 8 || p.stat_rows != p.mtiles * (p.TH / 8)) fail("one statistics row per 8 tile rows", s, f1, f2, p.stat_rows, p.mtiles);
        if (p.last_rows != -1) fail("last-pass rows outside linear tiles", s, f1, f2, p.last_rows, 0);
    }
    if (p.stat_rows > published_bound(s.N, s.H, s.W, s.Cout)) fail("statistics rows beyond ustrun_conv_mtiles", s, f1, f2, p.stat_rows, published_bound(s.N, s.H, s.W, s.Cout));
    // the build's own constraints
    if (p.pool != (s.kind == 2) || p.xf != (s.kind != 0) || p.dil != s.dil) fail("sources", s, f1, f2, p.xf, p.pool);
    if (p.bns && !(p.m16 && p.breg && !p.xf)) fail("sums need the 16x16x32 build on a plain source", s, f1, f2, p.m16, p.xf);
    if (p.bns != (s.bny && p.bns_ok)) fail("sums: bns = bny and eligible", s, f1, f2, p.bns, p.bns_ok);
    if (p.m16 && (p.xf || !p.breg)) fail("16x16x32: plain source, register-fed weights", s, f1, f2, p.xf, p.breg);
    if ((f1 & HALO_DBG_LDS_WEIGHTS) && p.breg) fail("flag: weights through LDS", s, f1, f2, p.breg, 0);
    if ((f1 & (HALO_DBG_M16_NONE | HALO_DBG_LDS_WEIGHTS)) && (p.m16 || p.bns_ok)) fail("flag: no 16x16x32", s, f1, f2, p.m16, p.bns_ok);
    if ((f2 & HALO_DBG2_NO_LINEAR) && p.linw) fail("flag: no linear tiles", s, f1, f2, p.linw, 0);
    return true;
}

static const int Ns[] = {1, 2, 3, 8, 9, 16, 17, 64}, HWs[] = {8, 16, 18, 20, 24, 33, 36, 48, 56, 64, 72, 96, 128, 144};
static const int Cs[][2] = {{64, 64}, {128, 64}, {128, 128}, {128, 512}, {512, 128}, {512, 512}, {1024, 1024}};
static const int FORCE1 = 1 << HALO_DBG_FORCE_SHIFT;
static const int Fs[][2] = {{0, 0}, {HALO_DBG_LDS_WEIGHTS, 0}, {FORCE1, 0}, {2 * FORCE1, 0}, {3 * FORCE1, 0}, {HALO_DBG_TILE512, 0},
                            {HALO_DBG_M16_ALL, 0}, {HALO_DBG_M16_NONE, 0}, {0, HALO_DBG2_NO_LINEAR},
                            // (no single flag reaches the 512-pixel tile's builds with weights through LDS / plain on 32x32x16)
                            {HALO_DBG_TILE512 | HALO_DBG_LDS_WEIGHTS, 0}, {HALO_DBG_TILE512 | HALO_DBG_M16_NONE, 0}};

static void expect(const char* what, bool ok, const Spec& s, const HaloPlan& p) { if (!ok) fail(what, s, 0, 0, p.variant, p.stat_rows); }

int main(int argc, char** argv) {
    bool print = false;
    long plans = 0, refused = 0, pins = 0;
    for (int i = 1; i < argc; ++i) {
        int v[12];
        if (!std::strcmp(argv[i], "rows")) { print = true; continue; }
        if (std::sscanf(argv[i], "pin=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11) != 12) {
            std::printf("bad argument %s\n", argv[i]);
            return 2;
        }
        const int gN = v[6] > 1 ? v[0] / v[6] : 0;
        HaloPlan p;
        const Spec fwd = {v[0], v[4], v[5], v[1], v[2], v[3], 1, v[7] ? 0 : 1, gN, 0, 0};
        if (!check_plan(fwd, v[8], v[9], &p) || p.variant != v[10]) fail("pinned forward variant", fwd, v[8], v[9], p.variant, v[10]);
        const Spec bwd = {v[0], v[4], v[5], v[3], 0, v[1] + v[2], 1, 0, 0, 0, 1};
        if (!check_plan(bwd, v[8], v[9], &p) || p.variant != v[11]) fail("pinned input-gradient variant", bwd, v[8], v[9], p.variant, v[11]);
        ++pins;
    }
    for (auto& b : g_builds) b.hits = 0;       // (the sweep's reach is counted without the pinned cases)

    for (int N : Ns) for (int H : HWs) for (int dW = 0; dW <= 8; dW += 8) for (auto& C : Cs) for (int two = 0; two < 2; ++two)
    for (int kind = 0; kind < 3; ++kind) for (int dil = 1; dil <= 4; dil *= 2) for (int bny = 0; bny < 2; ++bny) for (int div = 1; div <= 4; div *= 2) {
        if (N % div) continue;
        const Spec s = {N, H, H + dW, two ? C[0] / 2 : C[0], two ? C[0] / 2 : 0, C[1], dil, kind, div > 1 ? N / div : 0, bny, bny};
        for (auto& F : Fs) {
            HaloPlan p;
            if (!check_plan(s, F[0], F[1], &p)) { ++refused; continue; }
            ++plans;
            if (print && !two && kind != 1 && !bny && div == 1)
                std::printf("rows %d %d %d %d %d %d %d %d %d %d\n", N, s.H, s.W, C[0], C[1], dil, kind == 2, F[0], F[1], p.stat_rows);
        }
    }
    std::printf("sweep: %ld plans, %ld launches refused by halo_plan_supported, %ld pinned layers\n", plans, refused, pins);
    for (const Build& b : g_builds) {
        std::printf("build %-60s %8ld plans\n", b.name, b.hits);
        if (b.hits == 0) { ++g_fail; std::printf("FAIL the sweep never reached build %s\n", b.name); }
    }

    // literals (tests/test_host_logic.py pins the same launches through the library)
    {
        HaloPlan p;
        Spec s = {64, 18, 18, 1024, 0, 1024, 1, 0, 0, 0, 0};
        check_plan(s, 0, 0, &p);
        expect("64 x 18 x 18, 1024 -> 1024: linear tiles, ceil(64 * 19 * 19 / 256) rows", p.linw == 18 && p.stat_rows == (64 * 19 * 19 + 255) / 256, s, p);
        s.N = 1; check_plan(s, 0, 0, &p);
        expect("1 x 18 x 18, 1024 -> 1024: 6 rows on the 8 x 16 x 64 tile", p.TH == 8 && p.TW == 16 && p.BN == 64 && p.stat_rows == 6, s, p);
        s = {16, 48, 48, 512, 0, 512, 1, 0, 0, 0, 0}; check_plan(s, 0, 0, &p);
        expect("16 x 48 x 48, 512 -> 512: the 16 x 16 tile", p.TH == 16 && p.TW == 16 && p.BN == 128 && p.MI == 4, s, p);
        s = {8, 72, 72, 64, 0, 64, 1, 0, 0, 0, 0}; check_plan(s, 0, 0, &p);     // (the streaming 64 -> 64 kernel takes this launch: 432 rows)
        expect("8 x 72 x 72, 64 -> 64: 216 rows were it the halo's", p.stat_rows == 216, s, p);
        std::printf("pinned: four literals\n");
    }

    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
