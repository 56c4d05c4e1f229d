// convT_plan_check.hip -- host-only check of the plan of the pixel-linear GEMM family (ust-run_amd/csrc/convT_plan.h: the ConvTranspose forward,
// its input gradient, the 1x1 convolution with join / sums, and the ConvTranspose weight gradient) over a sweep of shapes, sources, pass
// groupings and the two debug flags (tests/test_convT_plan_host.py builds and runs it; no GPU, no device code is called).  Exit status 0 =
// every check passed.  Arguments:
//   rows                                     also print "rows N H W Cin Cout flags stat_rows" for every swept launch ustrun_debug_conv_stat_rows can
//                                            express (the 1x1 of a plain dense source), and "wg Cin Cout npix bytes" = ksplit x (slab + bias row) of
//                                            every planned weight gradient, for ustrun_wgrad_partials_bytes(4, Cin, Cout, npix)
//   pin1x1=N,H,W,Cin,Cout,flags,code         the 1x1 of a BatchNorm + ReLU source with statistics must plan this variant code
//   pinwg=N,Cin,Cout,H,W,G,xf,flags,code     the weight gradient (G passes, xf: BatchNorm + ReLU source) must plan this variant code
//   pindg=N,G,Cin,Cout,H,W,code              the input gradient with sums (Cin = channels of da) must plan this code; -1: sums not covered
//   pinct=N,G,Cin,Cout,H,W,flags,vf,vd       the ConvTranspose forward (G passes) and its input gradient must plan the codes vf / vd
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include "../../ust-run_amd/csrc/convT_plan.h"

using namespace ustrun;

static long g_fail = 0;
// kind as ConvTKind; src: 0 plain, 1 BatchNorm + ReLU on load; gN: images per pass (0: one pass); side: bit 0 join_add, 1 join_ref, 2 bny
struct Spec { int kind, N, H, W, Cin, Cout, src, gN, side; };
static void fail(const char* what, const Spec& s, int f, long a, long b) {
    if (g_fail++ < 20)
        std::printf("FAIL %s (kind %d, N = %d, %d x %d, %d -> %d, src %d, gN %d, side %d, flags %d): %ld, %ld\n", what, s.kind, s.N, s.H, s.W, s.Cin, s.Cout,
                    s.src, s.gN, s.side, f, a, b);
}
static const void* const P = (const void*)16;      // any non-null pointer: the plan never dereferences

static SrcDev dense(int C, int H, int W, int xf, int gN) {
    ustrun_src_t d = {};
    d.ptr = P; d.C = C; d.H = H; d.W = W;
    d.sC = 1; d.sW = C; d.sH = (int64_t)W * C; d.sN = (int64_t)H * d.sH;
    if (xf) { d.scale = d.shift = (const float*)P; d.relu = 1; }
    d.gN = gN; d.gstride = 4 * C;
    return make_src(d, USTRUN_D16);
}
// the launches as ops.hip / resnet_ops.hip describe them (s.Cin -> s.Cout in the direction of the GEMM: the gradient's Cin is du's channels)
static IgemmArgs make_args(const Spec& s) {
    IgemmArgs a = {};
    const bool dg = s.kind == CONVT_DGRAD;
    a.nsrc = 1; a.src[0] = dg ? dense(s.Cin, 2 * s.H, 2 * s.W, 0, 0) : dense(s.Cin, s.H, s.W, s.src, s.gN);
    a.Cin = s.Cin; a.W = (const float*)P; a.Cout = s.Cout;
    a.N = s.N; a.Hb = s.H; a.Wb = s.W; a.M = s.N * s.H * s.W;
    a.s_in = dg ? 2 : 1; a.nseg = dg ? 4 : 1; a.segw = dg ? 2 : 1; a.dstep = dg;
    a.nz = s.kind == CONVT_FWD ? 4 : 1; a.s_out = s.kind == CONVT_FWD ? 2 : 1;
    a.out0 = (float*)P; a.C0 = s.Cout; a.Ho = a.s_out * s.H; a.Wo = a.s_out * s.W; a.out_esz = 2;
    if (s.kind == CONVT_FWD) a.bias = (const float*)P;
    if (s.kind == CONVT_1X1 && !s.side) a.stat = (float*)P;
    if (s.side & 1) a.join_add = P;
    if (s.side & 2) a.join_ref = P;
    if (s.side & 4) { a.bny = P; a.bnsc = a.bnsh = (const float*)P; a.stat = (float*)P; a.bn_gN = s.gN; a.bn_gstride = 4 * s.Cout; }
    return a;
}

// the one list of builds, as the dispatch has it: key, ConvTGeom's LDS bytes, and how often the sweep reached each
struct Build { long key; int lds; const char* name; long hits; };
#define ROW(BN, BK, MODE, BREG, BNS, JOIN) \
    {convT_key(BN, BK, MODE, BREG, BNS, JOIN), ConvTGeom<BN, BK, MODE, BREG, BNS, JOIN>::lds, "convT<" #BN "," #BK "," #MODE "," #BREG "," #BNS "," #JOIN ">", 0},
static Build g_builds[] = {CONVT_BUILDS(ROW)};
#undef ROW
#define R1() {1, WGT_LDS, "wgradT", 0},
#define RT(TM, DIAG) {2 * TM + DIAG, T2<TM>::lds, "wgradT2<" #TM "," #DIAG ">", 0},
static Build g_wbuilds[] = {WGRADT_BUILDS(R1, RT)};
#undef R1
#undef RT

static int published_bound(int N, int H, int W, int Cout) {       // ustrun_conv_mtiles (ops.hip)
    const int lin = cdiv((int64_t)N * H * W, 128), tiled = N * cdiv(H, 16) * 2 * cdiv(W, 16), stream = Cout == 64 ? 2 * N * cdiv(W, 32) * cdiv(H, 8) : 0;
    const int m = lin > tiled ? lin : tiled;
    return m > stream ? m : stream;
}

// every property one plan must have; returns false when the family does not take the launch
static bool check_plan(const Spec& s, int f, ConvTPlan* out = nullptr) {
    const IgemmArgs a = make_args(s);
    const ConvTPlan p = convT_plan(a, f);
    if (out) *out = p;
    if (p.kind == CONVT_NONE) return false;
    const bool joined = (s.side & 7) && s.kind == CONVT_1X1;
    if (p.kind != (joined && p.join_ok ? (int)CONVT_1X1_JOIN : s.kind)) fail("kind", s, f, p.kind, s.kind);
    // the build exists, with ConvTGeom's LDS size, inside the 160 KB of a CU
    Build* b = nullptr;
    for (Build& g : g_builds) if (g.key == p.key) b = &g;
    if (!b) { fail("the plan names no build of the dispatch", s, f, p.variant, p.key >> 32); return true; }
    ++b->hits;
    if (p.lds != b->lds || p.lds <= 0 || p.lds > 160 * 1024) fail("LDS bytes", s, f, p.lds, b->lds);
    if (p.key != convT_key(p.BN, p.BK, p.MODE, p.breg, p.bns, p.join) || p.variant != (int)(p.key & 0xffffffffL)) fail("key / variant", s, f, p.variant, p.key);
    // tiles, grid and statistics rows
    const int ncols = p.MODE == 0 ? 4 * s.Cout : s.Cout;
    if (p.mt != cdiv(a.M, 128) || p.nt * p.BN != ncols || p.grid != p.mt * p.nt) fail("tiles", s, f, p.mt, p.nt);
    if (p.stat_rows != cdiv(a.M, 128) || p.stat_rows > published_bound(s.N, s.H, s.W, s.Cout)) fail("statistics rows", s, f, p.stat_rows, published_bound(s.N, s.H, s.W, s.Cout));
    // a 128-pixel tile lies inside one pass where the kernel picks per-pass constants: the forward's source, the gradient's sums
    const long gpix = (long)s.gN * s.H * s.W;
    if (p.kind == CONVT_FWD && s.gN > 0 && gpix % 128) fail("forward tile straddles a pass", s, f, gpix, 0);
    if (p.kind == CONVT_DGRAD && p.bns_ok && s.gN > 0 && (s.side & 4) && gpix % 128) fail("sums tile straddles a pass", s, f, gpix, 0);
    if (p.kind != CONVT_FWD && p.kind != CONVT_DGRAD && s.gN > 0) fail("the 1x1 takes one pass", s, f, s.gN, 0);
    // the builds' own constraints and the flag
    const bool lds_w = f & CONVT_DBG_LDS_WEIGHTS;
    if (p.breg == lds_w) fail("flag: weights through LDS / registers", s, f, p.breg, lds_w);
    if (lds_w && (p.bns || p.join || p.bns_ok || p.join_ok)) fail("flag: no sums, no join on the LDS-weight builds", s, f, p.bns, p.join);
    if (p.bns != ((s.side & 4) && (p.join || p.bns_ok))) fail("sums: bny and eligible", s, f, p.bns, p.bns_ok);
    if (p.join && (s.src || s.Cout % 128)) fail("join: plain source, 128-column tiles", s, f, s.src, s.Cout);
    if (p.BN == 256 && (long)p.mt * (s.Cout / 256) < (p.kind == CONVT_DGRAD ? 512 : p.kind == CONVT_FWD ? 0 : 256)) fail("wide tile below its block count", s, f, p.mt, s.Cout);
    return true;
}

static WgradArgs make_wargs(int N, int H, int W, int Cin, int Cout, int xf, int gN) {
    WgradArgs a = {};
    a.nsrc = 1; a.src[0] = dense(Cin, H, W, xf, gN); a.Cin = Cin;
    a.dy = (const float*)P; a.Cout = Cout; a.dy_esz = 2;
    a.N = N; a.Hb = H; a.Wb = W; a.M = (long)N * H * W;
    a.nseg = 4; a.segw = 2; a.dy_s = 2; a.dyH = 2 * H; a.dyW = 2 * W;
    return a;
}
static bool check_wplan(int N, int H, int W, int Cin, int Cout, int xf, int gN, int f, bool print, WgradTPlan* out = nullptr) {
    const WgradArgs a = make_wargs(N, H, W, Cin, Cout, xf, gN);
    const WgradTPlan p = wgradT_plan(a, f);
    if (out) *out = p;
    if (!p.ok) return false;
    const Spec s = {0, N, H, W, Cin, Cout, xf, gN, 0};
    const long gpix = (long)gN * H * W;
    Build* b = nullptr;
    for (Build& g : g_wbuilds) if (g.key == (p.kernel == 1 ? 1 : 2 * p.tm)) b = &g;
    if (!b) { fail("the plan names no weight-gradient build", s, f, p.kernel, p.tm); return true; }
    ++b->hits;
    if (p.lds != b->lds || p.lds > 160 * 1024) fail("weight gradient: LDS bytes", s, f, p.lds, b->lds);
    if (p.kernel == 2 ? ((f & WGRADT_DBG_ROUND1) || Cout % 64 || Cin % p.tm || W < 16 || p.stage != 32 || p.cols != 64 || p.threads != 2 * p.tm ||
                         p.variant != (0x54320000 | p.tm) || p.tm != (Cin % 256 ? 128 : 256))
                      : (Cin % 128 || Cout % 32 || p.tm != 128 || p.stage != 64 || p.cols != 32 || p.threads != 256 || p.variant != 0x54310000 ||
                         (!(f & WGRADT_DBG_ROUND1) && Cout % 64 == 0 && W >= 16 && gpix % 32 == 0)))
        fail("weight gradient: which kernel", s, f, p.kernel, p.tm);
    if (gpix % p.stage) fail("weight gradient: a stage straddles a pass", s, f, gpix, p.stage);
    if (p.ksplit < 1 || p.kchunk % p.stage || p.ksplit * p.kchunk < a.M || (p.ksplit - 1) * p.kchunk >= a.M) fail("weight gradient: split-K covers the pixels", s, f, p.ksplit, p.kchunk);
    if (p.grid != (Cin / p.tm) * (Cout / p.cols) * p.ksplit) fail("weight gradient: grid", s, f, p.grid, p.ksplit);
    if (p.ksplit > wgradT_max_ksplit(Cin, Cout, a.M)) fail("weight gradient: ksplit beyond the published maximum", s, f, p.ksplit, wgradT_max_ksplit(Cin, Cout, a.M));
    if (print) std::printf("wg %d %d %ld %ld\n", Cin, Cout, a.M, (long)p.ksplit * (4L * Cin * Cout + Cout) * 4);
    return true;
}

static const int Ns[] = {1, 2, 3, 8, 64};
static const int HWs[][2] = {{3, 5}, {5, 7}, {9, 11}, {12, 15}, {16, 16}, {20, 24}, {18, 18}, {64, 64}, {9, 144}, {1, 32768}, {2, 40000}};
static const int Cs[][2] = {{64, 64}, {128, 64}, {64, 128}, {256, 128}, {128, 96}, {192, 192}, {512, 256}, {256, 512}, {1024, 512}, {256, 1024}, {100, 64}, {128, 48}, {64, 32}};
static const int Fs[] = {0, CONVT_DBG_LDS_WEIGHTS, WGRADT_DBG_ROUND1, CONVT_DBG_LDS_WEIGHTS | WGRADT_DBG_ROUND1};

int main(int argc, char** argv) {
    bool print = false;
    long plans = 0, refused = 0, wplans = 0, pins = 0;
    for (int i = 1; i < argc; ++i) {
        int v[9];
        ConvTPlan p;
        WgradTPlan w;
        if (!std::strcmp(argv[i], "rows")) { print = true; continue; }
        if (std::sscanf(argv[i], "pin1x1=%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) == 7) {
            const Spec s = {CONVT_1X1, v[0], v[1], v[2], v[3], v[4], 1, 0, 0};
            if (!check_plan(s, v[5], &p) || p.variant != v[6]) fail("pinned 1x1 variant", s, v[5], p.variant, v[6]);
        } else if (std::sscanf(argv[i], "pinwg=%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 9) {
            const Spec s = {0, v[0], v[3], v[4], v[1], v[2], v[6], v[5] > 1 ? v[0] / v[5] : 0, 0};
            if (!check_wplan(s.N, s.H, s.W, s.Cin, s.Cout, s.src, s.gN, v[7], false, &w) || w.variant != v[8]) fail("pinned weight-gradient variant", s, v[7], w.variant, v[8]);
        } else if (std::sscanf(argv[i], "pindg=%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) == 7) {
            const Spec s = {CONVT_DGRAD, v[0], v[4], v[5], v[3], v[2], 0, v[1] > 1 ? v[0] / v[1] : 0, 4};
            const bool took = check_plan(s, 0, &p);
            if (!took || (v[6] == -1 ? p.bns_ok : (!p.bns || p.variant != v[6]))) fail("pinned input gradient with sums", s, 0, p.variant, v[6]);
        } else if (std::sscanf(argv[i], "pinct=%d,%d,%d,%d,%d,%d,%d,%d,%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 9) {
            const Spec sf = {CONVT_FWD, v[0], v[4], v[5], v[2], v[3], 1, v[1] > 1 ? v[0] / v[1] : 0, 0}, sd = {CONVT_DGRAD, v[0], v[4], v[5], v[3], v[2], 0, 0, 0};
            // (passes that are no multiple of 128 pixels: ustrun_convT2x2_fwd runs the forward once per pass)
            const Spec s1 = {CONVT_FWD, v[0] / v[1], v[4], v[5], v[2], v[3], 1, 0, 0};
            if (!(check_plan(sf, v[6], &p) || check_plan(s1, v[6], &p)) || p.variant != v[7]) fail("pinned forward variant", sf, v[6], p.variant, v[7]);
            if (!check_plan(sd, v[6], &p) || p.variant != v[8]) fail("pinned input-gradient variant", sd, v[6], p.variant, v[8]);
        } else { std::printf("bad argument %s\n", argv[i]); return 2; }
        ++pins;
    }
    for (Build& b : g_builds) b.hits = 0;        // (the sweep's reach is counted without the pinned cases)
    for (Build& b : g_wbuilds) b.hits = 0;

    for (int N : Ns) for (auto& hw : HWs) for (auto& C : Cs) for (int div = 1; div <= 4; div *= 2) for (int f : Fs) {
        if (N % div) continue;
        const int H = hw[0], W = hw[1], gN = div > 1 ? N / div : 0;
        for (int src = 0; src < 2; ++src) {
            const Spec fwd = {CONVT_FWD, N, H, W, C[0], C[1], src, src ? gN : 0, 0};
            check_plan(fwd, f) ? ++plans : ++refused;
            wplans += check_wplan(N, H, W, C[0], C[1], src, src ? gN : 0, f, print);
            for (int side : {0, 1, 2, 3, 4, 7}) {
                if (div > 1) continue;
                const Spec one = {CONVT_1X1, N, H, W, C[0], C[1], src, 0, side};
                ConvTPlan p;
                if (!check_plan(one, f, &p)) { ++refused; continue; }
                ++plans;
                if (print && !src && !side) std::printf("rows %d %d %d %d %d %d %d\n", N, H, W, C[0], C[1], f, p.stat_rows);
            }
        }
        for (int bny = 0; bny < 2; ++bny) {
            const Spec dg = {CONVT_DGRAD, N, H, W, C[1], C[0], 0, bny ? gN : 0, bny ? 4 : 0};      // da has the forward's Cin channels
            check_plan(dg, f) ? ++plans : ++refused;
        }
    }
    std::printf("sweep: %ld GEMM plans, %ld launches left to other kernels, %ld weight-gradient plans, %ld pinned cases\n", plans, refused, wplans, pins);
    for (const Build& b : g_builds) {
        std::printf("build %-40s %8ld plans\n", b.name, b.hits);
        if (b.hits == 0) { ++g_fail; std::printf("FAIL the sweep never reached build %s\n", b.name); }
    }
    // the DIAG build (phase stamps) is no plan's choice: wgradT_launch_bf16 takes it in place of wgradT2<256,0> while ustrun_debug_buffer is set,
    // so it is reached exactly where that build is
    for (Build& b : g_wbuilds) {
        if (!std::strcmp(b.name, "wgradT2<256,1>")) for (const Build& o : g_wbuilds) if (!std::strcmp(o.name, "wgradT2<256,0>")) b.hits = o.hits;
        std::printf("build %-40s %8ld plans\n", b.name, b.hits);
        if (b.hits == 0) { ++g_fail; std::printf("FAIL the sweep never reached build %s\n", b.name); }
    }
    // extents the family must leave to the generic kernel
    {
        ConvTPlan p;
        const Spec big = {CONVT_1X1, 1, 1, 32768, 64, 64, 0, 0, 0}, odd = {CONVT_FWD, 2, 9, 11, 100, 64, 0, 0, 0}, pass = {CONVT_FWD, 6, 10, 12, 128, 64, 1, 3, 0};
        if (check_plan(big, 0, &p)) fail("W >= 32768 must be refused", big, 0, p.kind, 0);
        if (check_plan(odd, 0, &p)) fail("Cin % 64 != 0 must be refused", odd, 0, p.kind, 0);
        if (check_plan(pass, 0, &p)) fail("a forward whose passes are no multiple of 128 pixels must be refused", pass, 0, p.kind, 0);
        std::printf("pinned: three refusals\n");
    }
    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
