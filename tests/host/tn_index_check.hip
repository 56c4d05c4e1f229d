// tn_index_check.hip -- host-only check of the index helpers and the tile cursor of ust-run_amd/csrc/tn_gemm.h over the domains their comments claim
// (tests/test_tn_index_host.py builds and runs it; no GPU, no device code is called).  Exit status 0 = every check passed.
#include <cstdio>
#include <vector>
#include "../../ust-run_amd/csrc/tn_gemm.h"

using namespace ustrun;

static long g_fail = 0;
static void fail(const char* what, long a, long b, long c, long got, long want) {
    if (g_fail++ < 20) std::printf("FAIL %s(%ld, %ld, %ld): got %ld, want %ld\n", what, a, b, c, got, want);
}

static void check_fdiv(int v, int d, float invd) {
    int rem = -1;
    const int q = fdiv(v, d, invd, rem);
    if (q != v / d) fail("fdiv quotient", v, d, 0, q, v / d);
    if (rem != v % d) fail("fdiv remainder", v, d, 0, rem, v % d);
}

int main() {
    constexpr int VMAX = 1 << 24;

    // fdiv over the whole range 0 <= v < 2^24
    const int full[] = {1, 2, 3, 5, 7, 9, 12, 13, 16, 17, 18, 24, 32, 33, 36, 48, 64, 65, 72, 96, 128, 129, 144, 192, 256, 257, 288, 384, 512, 513};
    long n_full = 0;
    for (int d : full) {
        const float invd = 1.f / (float)d;
        for (int v = 0; v < VMAX; ++v) check_fdiv(v, d, invd);
        n_full += VMAX;
    }
    std::printf("fdiv full range: %zu divisors, %ld cases\n", sizeof(full) / sizeof(full[0]), n_full);

    // fdiv at every multiple of d and its two neighbours
    long n_edge = 0;
    for (int d = 1; d <= 4096; ++d) {
        const float invd = 1.f / (float)d;
        for (long m = 0; m - 1 < VMAX; m += d)
            for (long v = m - 1; v <= m + 1; ++v)
                if (v >= 0 && v < VMAX) { check_fdiv((int)v, d, invd); ++n_edge; }
    }
    std::printf("fdiv boundaries: d = 1..4096, %ld cases\n", n_edge);

    // wrap_add: x in the first and the last 65 values of [0, W)
    long n_wrap = 0;
    for (int W = 1; W <= 32767; ++W) {
        const float invW = 1.f / (float)W;
        for (int x = 0; x < W; ++x) {
            if (x >= 65 && x < W - 65) { x = W - 65 - 1; continue; }
            for (int inc = 0; inc <= 64; ++inc) {
                const int got = wrap_add(x, inc, W, invW);
                if (got != (x + inc) % W) fail("wrap_add", x, inc, W, got, (x + inc) % W);
                ++n_wrap;
            }
        }
    }
    std::printf("wrap_add: W = 1..32767, %ld cases\n", n_wrap);

    // xcd_linear: a permutation of [0, nblk) in which the blocks of one XCD (bid % 8 == x) take one contiguous range
    std::vector<char> seen;
    for (int nblk = 1; nblk <= 4100; ++nblk) {
        seen.assign(nblk, 0);
        for (int x = 0; x < 8; ++x) {
            int lo = nblk, hi = -1, cnt = 0;
            for (int bid = x; bid < nblk; bid += 8) {
                const int lin = xcd_linear((unsigned)bid, nblk);
                if (lin < 0 || lin >= nblk) { fail("xcd_linear range", bid, nblk, 0, lin, -1); continue; }
                if (seen[lin]++) fail("xcd_linear twice", bid, nblk, 0, lin, -1);
                lo = lin < lo ? lin : lo; hi = lin > hi ? lin : hi; ++cnt;
            }
            if (cnt && hi - lo + 1 != cnt) fail("xcd_linear contiguous", x, nblk, cnt, hi - lo + 1, cnt);
        }
        for (int i = 0; i < nblk; ++i)
            if (!seen[i]) fail("xcd_linear missing", i, nblk, 0, 0, 1);
    }
    std::printf("xcd_linear: nblk = 1..4100\n");

    // tile_cursor: seek(t) is image t / (ty tx), column (t mod ty tx) / ty, row t mod ty (y fastest), and k advances from seek(t0)
    // -- one per step, or two as the two-group kernel takes them -- land on seek(t0 + k stride), up to the last tile
    long n_cur = 0;
    const int dims[] = {1, 2, 3, 5, 8};
    for (int N : {1, 3})
        for (int ty : dims)
            for (int tx : dims) {
                const int total = N * ty * tx;
                for (int stride = 1; stride <= 2; ++stride)
                    for (int t0 = 0; t0 < total; ++t0) {
                        tile_cursor<8, 16> c;
                        c.seek(t0, ty, tx);
                        for (int t = t0; t < total; t += stride) {
                            tile_cursor<8, 16> w;
                            w.seek(t, ty, tx);
                            const int img = t / (ty * tx), col = (t % (ty * tx)) / ty, row = t % ty;
                            if (w.img != img || w.x0 != col * 16 || w.y0 != row * 8) fail("tile_cursor seek", t, ty, tx, w.img * 10000 + w.x0 * 10 + w.y0, img * 10000 + col * 160 + row * 8);
                            if (c.img != w.img || c.y0 != w.y0 || c.x0 != w.x0 || c.yend != w.yend || c.xend != w.xend)
                                fail(stride == 1 ? "tile_cursor advance x1" : "tile_cursor advance x2", t0, t, ty * 100 + tx, c.img * 10000 + c.x0 * 10 + c.y0, w.img * 10000 + w.x0 * 10 + w.y0);
                            ++n_cur;
                            for (int s_ = 0; s_ < stride; ++s_) c.advance();
                        }
                    }
            }
    std::printf("tile_cursor: tiles 1..8 x 1..8, N = 1 and 3, strides 1 and 2, %ld positions\n", n_cur);

    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
