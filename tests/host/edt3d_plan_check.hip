// edt3d_plan_check.hip -- host-only replay of ust-run_amd/csrc/edt3d_plan.h (tests/test_edt3d_host.py builds and runs it; no GPU,
// no device code is called): the limits and the overflow bound at their edges, the percentile ranks, the grid folding, the radix
// digits driving a three-level select, and the two searches (row_min, z_min) run in the kernels' pass order over small volumes
// against a brute force in int64.  Exit status 0 = every check passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../ust-run_amd/csrc/edt3d_plan.h"

using namespace ustrun::edt3d;

static long g_fail = 0;
static void fail(const char* what, long a, long b, long c, long got, long want) {
    if (g_fail++ < 20) std::printf("FAIL %s(%ld, %ld, %ld): got %ld, want %ld\n", what, a, b, c, got, want);
}

static unsigned g_seed = 12345;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// the column pass the kernels take from edt_scan.h, restated: distance along y to the nearest source, COL_CAP without one
static void colscan(int H, int W, std::vector<unsigned short>& m) {
    for (int x = 0; x < W; ++x) {
        int d = COL_CAP;
        for (int y = 0; y < H; ++y) { d = m[y * W + x] == 0 ? 0 : std::min(d + 1, COL_CAP); m[y * W + x] = (unsigned short)d; }
        d = COL_CAP;
        for (int y = H - 1; y >= 0; --y) { d = std::min((int)m[y * W + x], std::min(d + 1, COL_CAP)); m[y * W + x] = (unsigned short)d; }
    }
}

// g2 of every voxel to the set `src` [D][H][W] within its slice (passes 1-3), G_NONE in a slice without a source
static std::vector<int> slice_g2(const std::vector<char>& src, int D, int H, int W, int wy, int wx) {
    std::vector<int> g((size_t)D * H * W);
    for (int z = 0; z < D; ++z) {
        std::vector<unsigned short> col((size_t)H * W);
        for (int i = 0; i < H * W; ++i) col[i] = src[(size_t)z * H * W + i] ? 0 : COL_CAP;
        colscan(H, W, col);
        for (int y = 0; y < H; ++y) {
            bool any = false;
            for (int x = 0; x < W; ++x) any |= col[y * W + x] < COL_CAP;
            for (int x = 0; x < W; ++x) g[((size_t)z * H + y) * W + x] = row_min(&col[y * W], x, W, wy * wy, wx * wx, any);
        }
    }
    return g;
}

static long long brute(const std::vector<char>& src, int D, int H, int W, int wz, int wy, int wx, int z, int y, int x) {
    long long best = -1;
    for (int c = 0; c < D; ++c)
        for (int b = 0; b < H; ++b)
            for (int a = 0; a < W; ++a)
                if (src[((size_t)c * H + b) * W + a]) {
                    const long long d = (long long)wz * wz * (z - c) * (z - c) + (long long)wy * wy * (y - b) * (y - b) + (long long)wx * wx * (x - a) * (x - a);
                    if (best < 0 || d < best) best = d;
                }
    return best;
}

static long check_volume(int D, int H, int W, int wz, int wy, int wx, int density) {
    const size_t n = (size_t)D * H * W;
    const long HW = (long)H * W;
    std::vector<char> fg(n), bg(n);
    size_t nfg = 0;
    for (size_t i = 0; i < n; ++i) { fg[i] = density == 0 ? (i == 0) : (int)(rnd() % 100) < density; bg[i] = !fg[i]; nfg += fg[i]; }
    if (density == 1) { std::fill(fg.begin(), fg.end(), 0); std::fill(bg.begin(), bg.end(), 1); nfg = 0;      // one slice only holds sources
        for (long i = 0; i < HW; ++i) if (rnd() % 3 == 0) { fg[(size_t)(D / 2) * HW + i] = 1; bg[(size_t)(D / 2) * HW + i] = 0; ++nfg; } }
    // the surface form: two dense maps, the search at every voxel to the set fg
    const std::vector<int> gf = slice_g2(fg, D, H, W, wy, wx), gb = slice_g2(bg, D, H, W, wy, wx);
    // the signed form: one map, + g2 to the slice's foreground on background, - g2 to its background on foreground
    std::vector<int> sg(n);
    for (size_t i = 0; i < n; ++i) sg[i] = fg[i] ? -gb[i] : gf[i];
    for (size_t i = 0; i < n; ++i) if (sg[i] == 0) fail("signed map holds 0", (long)i, 0, 0, 0, 1);
    long checked = 0;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t e = ((size_t)z * H + y) * W + x;
                if (nfg) {
                    const int got = z_min<false>(&gf[e], z, D, HW, wz * wz, gf[e], false);
                    const long long want = brute(fg, D, H, W, wz, wy, wx, z, y, x);
                    if (got != want) fail("z_min dense", z, y, x, got, (long)want);
                    ++checked;
                }
                const bool f = fg[e];
                if (f ? nfg < n : nfg > 0) {
                    const int got = z_min<true>(&sg[e], z, D, HW, wz * wz, f ? -sg[e] : sg[e], f);
                    const long long want = brute(f ? bg : fg, D, H, W, wz, wy, wx, z, y, x);
                    if (got != want) fail("z_min signed", z, y, x, got, (long)want);
                    ++checked;
                }
            }
    return checked;
}

int main() {
    // limits
    if (!sizes_ok(1, 1, 1, 1, 1) || !sizes_ok(1, 32767, 1024, 1024, 1024) || sizes_ok(1, 32768, 1, 1, 1) || sizes_ok(2, 16384, 1, 1, 1) ||
        sizes_ok(1, 1, 0, 1, 1) || sizes_ok(1, 1, 1, 1025, 1) || sizes_ok(1, 1, 1, 1, 1025) || sizes_ok(1, 1, 1025, 1, 1) || sizes_ok(0, 1, 1, 1, 1))
        fail("sizes_ok", 0, 0, 0, 0, 1);
    if (!voxels_ok(1024, 1024, 128) || voxels_ok(1024, 1024, 129) || voxels_ok(1024, 1024, 1024)) fail("voxels_ok", 0, 0, 0, 0, 1);
    if (!weights_ok(1, 255, 1) || weights_ok(0, 1, 1) || weights_ok(1, 256, 1) || weights_ok(1, 1, -1)) fail("weights_ok", 0, 0, 0, 0, 1);
    // the overflow bound at its edge: 45 * 1023 = 46035, 46035^2 = 2119221225 <= 2^31 - 2 < (46 * 1023)^2
    if (!d2_fits(1024, 1, 1, 45, 1, 1) || d2_fits(1024, 1024, 128, 46, 1, 1) || d2_fits(1024, 1, 1, 46, 1, 1)) fail("d2_fits edge", 0, 0, 0, 0, 1);
    if (d2_bound(1024, 1024, 1024, 255, 255, 255) != 3LL * 255 * 255 * 1023 * 1023) fail("d2_bound max", 0, 0, 0, 0, 1);
    if (!d2_fits(1024, 1024, 1024, 1, 1, 1) || !d2_fits(129, 8, 8, 255, 1, 1) || !d2_fits(40, 64, 64, 40, 1, 1)) fail("d2_fits", 0, 0, 0, 0, 1);
    // 46340^2 = 2147395600 <= 2^31 - 2 < 46341^2: the bound itself is exact
    if (!d2_fits(2, 1, 1, 1, 1, 1)) fail("d2_fits small", 0, 0, 0, 0, 1);
    long n_bound = 0;
    for (int D = 1; D <= 1024; D += 31)
        for (int w = 1; w <= 255; w += 2) {
            const long long b = (long long)w * w * (D - 1) * (D - 1) + 49LL * 9 + 25LL * 16;
            if (d2_bound(D, 4, 5, w, 7, 5) != b) fail("d2_bound", D, w, 0, (long)d2_bound(D, 4, 5, w, 7, 5), (long)b);
            if (d2_fits(D, 4, 5, w, 7, 5) != (b <= 2147483646LL)) fail("d2_fits", D, w, 0, 0, 1);
            ++n_bound;
        }
    std::printf("limits and overflow bound: %ld cases\n", n_bound);

    // ranks: floor(0.95 (n - 1)) in f64, as numpy takes it
    long n_rank = 0;
    for (long n = 1; n <= (1L << 28); n += (n < 100000 ? 1 : 9973)) {
        const int k = rank95((int)n), k1 = rank95_next((int)n);
        const double pos = 0.95 * (double)(n - 1);
        if (k != (int)std::floor(pos) || k < 0 || k >= n) fail("rank95", n, 0, 0, k, (long)std::floor(pos));
        if (k1 != (k + 1 < n ? k + 1 : n - 1)) fail("rank95_next", n, 0, 0, k1, k + 1);
        ++n_rank;
    }
    if (rank95(1 << 28) != (int)std::floor(0.95 * ((double)(1 << 28) - 1))) fail("rank95 top", 0, 0, 0, 0, 1);
    std::printf("ranks: %ld list lengths up to 2^28\n", n_rank);

    // folding: every item is visited exactly once, the block count respects the cap
    long n_fold = 0;
    for (int per : {1, 4})
        for (int cap : {1, 7, 65535})
            for (long items : {1L, 3L, 4L, 5L, 65535L, 65536L, 66000L, 262141L, 300000L}) {
                const int blocks = fold_blocks(items, per, cap);
                if (blocks < 1 || blocks > cap) fail("fold_blocks cap", items, per, cap, blocks, cap);
                std::vector<char> seen((size_t)items, 0);
                for (long b = 0; b < blocks; ++b)
                    for (long i0 = b * per; i0 < items; i0 += (long)blocks * per)
                        for (long i = i0; i < i0 + per && i < items; ++i) if (seen[(size_t)i]++) fail("fold twice", items, per, cap, i, -1);
                for (long i = 0; i < items; ++i) if (!seen[(size_t)i]) fail("fold missing", items, per, cap, i, -1);
                ++n_fold;
            }
    std::printf("folding: %ld (items, per, cap) triples\n", n_fold);

    // the digits: they rebuild the value, and a three-level histogram select finds every rank of a list
    for (int v : {0, 1, 1023, 1024, (1 << 20) - 1, 1 << 20, (1 << 21) + 5, 1 << 30, 2147483646}) {
        if (((digit1(v) << (L2_BITS + L3_BITS)) | (digit2(v) << L3_BITS) | digit3(v)) != v || digit1(v) >= (1 << L1_BITS) ||
            prefix2(v) != ((digit1(v) << L2_BITS) | digit2(v)))
            fail("digits", v, 0, 0, 0, 1);
    }
    long n_sel = 0;
    for (int trial = 0; trial < 40; ++trial) {
        const int n = 1 + rnd() % 300;
        std::vector<int> a(n);
        for (int& v : a) v = trial % 4 == 0 ? (int)(rnd() % 5) : (trial % 4 == 1 ? (int)((rnd() * 131u) % 2147483647u) : (int)(rnd() % (1 << 22)) + (trial % 4 == 3 ? (1 << 30) : 0));
        std::vector<int> s(a);
        std::sort(s.begin(), s.end());
        for (int rank : {rank95(n), rank95_next(n), 0, n - 1}) {
            int pre = 0, r = rank;
            for (int level = 1; level <= 3; ++level) {
                std::vector<int> hist(1 << L1_BITS, 0);
                for (int v : a) {
                    const bool in = level == 1 || (level == 2 ? digit1(v) == pre : prefix2(v) == pre);
                    if (in) ++hist[level == 1 ? digit1(v) : (level == 2 ? digit2(v) : digit3(v))];
                }
                int b = 0;
                while (r >= hist[b]) r -= hist[b++];
                pre = level == 1 ? b : ((pre << L2_BITS) | b);
            }
            if (pre != s[rank]) fail("select", n, rank, trial, pre, s[rank]);
            ++n_sel;
        }
    }
    std::printf("select: %ld ranks\n", n_sel);

    // the searches in pass order against the brute force
    long n_vox = 0;
    const int shapes[][3] = {{1, 1, 1}, {1, 7, 9}, {5, 1, 1}, {3, 5, 1}, {6, 10, 13}, {9, 5, 7}, {2, 2, 2}};
    const int weights[][3] = {{1, 1, 1}, {8, 1, 1}, {5, 2, 2}, {1, 3, 2}, {255, 1, 1}, {16, 5, 5}};
    for (const auto& sh : shapes)
        for (const auto& w : weights)
            for (int density : {0, 1, 5, 50, 95}) n_vox += check_volume(sh[0], sh[1], sh[2], w[0], w[1], w[2], density);
    n_vox += check_volume(129, 3, 2, 255, 1, 1, 0);
    n_vox += check_volume(130, 3, 2, 255, 1, 1, 0);          // 255^2 129^2: a value past 2^30
    n_vox += check_volume(40, 8, 8, 40, 1, 1, 0);
    std::printf("searches: %ld voxel distances over %zu shapes x %zu weights\n", n_vox, sizeof(shapes) / sizeof(shapes[0]),
                sizeof(weights) / sizeof(weights[0]));

    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
