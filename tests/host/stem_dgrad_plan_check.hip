// stem_dgrad_plan_check.hip -- host-only check of the tap and parity arithmetic of the 7x7 / stride-2 / padding-3 stem convolution's
// input gradient (ust-run_amd/csrc/stem_dgrad_plan.h) against brute force, for every H, W in 1..40 and every tile origin
// (tests/test_stem_dgrad_plan_host.py builds and runs it; no GPU, no device code is called).  Exit status 0 = every check passed.
//
// The kernel's walk is repeated here with the header's functions: tile (y0, x0) -> quad (ly, lx) -> parities (py, px) -> offsets
// (dy, dx) -> taps sd_tap_of -> patch indices sd_patch_index -> outputs sd_patch_origin + index.  Per input pixel the taps that land
// inside the output map must be exactly {(ky, kx): iy + 3 - ky and ix + 3 - kx even, ((iy + 3 - ky) / 2, (ix + 3 - kx) / 2) inside
// [0, Ho) x [0, Wo)}, each reading exactly that output; every index the walk touches, inside the map or not, must lie inside the
// SD_PATCH x SD_PATCH patch the plan declares; the tiles must cover every input pixel once.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../ust-run_amd/csrc/stem_dgrad_plan.h"

using namespace ustrun;

static long g_fail = 0;
static void fail(const char* what, int H, int W, long a, long b) {
    if (g_fail++ < 20) std::printf("FAIL %s (%d x %d): %ld, %ld\n", what, H, W, a, b);
}

// one axis by brute force, from the forward's definition: output o reads input 2 o - 3 + k
static uint32_t brute_axis(int i, int H, int Ho, int o_of_k[SD_K]) {
    uint32_t m = 0;
    for (int o = 0; o < Ho; ++o)
        for (int k = 0; k < SD_K; ++k)
            if (2 * o - SD_PAD + k == i) { m |= 1u << k; o_of_k[k] = o; }
    (void)H;
    return m;
}

int main() {
    long pixels = 0, taps = 0, touched = 0, outside = 0;
    // ---- the constants and the per-tap functions
    if (SD_T % 2 || SD_Q * 2 != SD_T || SD_PATCH != SD_Q + SD_DMAX - SD_DMIN) fail("constants", 0, 0, SD_T, SD_PATCH);
    for (int k = 0; k < SD_K; ++k) {
        const int p = sd_tap_parity(k), d = sd_tap_shift(k);
        if ((SD_PAD + p - k) % 2 || d < SD_DMIN || d > SD_DMAX || sd_tap_of(p, d) != k) fail("tap parity / shift / inverse", 0, 0, k, d);
    }
    int ntap = 0;
    for (int p = 0; p < 2; ++p)
        for (int d = SD_DMIN; d <= SD_DMAX; ++d) {
            const int k = sd_tap_of(p, d);
            if (k < 0) continue;
            ++ntap;
            if (k >= SD_K || sd_tap_parity(k) != p || sd_tap_shift(k) != d) fail("tap of (parity, shift)", 0, 0, p, d);
        }
    if (ntap != SD_K || sd_tap_of(0, SD_DMAX) != -1) fail("seven taps over two parities", 0, 0, ntap, 0);

    std::vector<int> cover;
    for (int H = 1; H <= 40; ++H)
        for (int W = 1; W <= 40; ++W) {
            const int Ho = sd_out_extent(H), Wo = sd_out_extent(W);
            if (Ho != (H + 2 * SD_PAD - SD_K) / 2 + 1 || Wo != (W + 2 * SD_PAD - SD_K) / 2 + 1) fail("output extent", H, W, Ho, Wo);
            cover.assign((size_t)H * W, 0);
            const int ty = sd_tiles(H), tx = sd_tiles(W);
            if ((ty - 1) * SD_T >= H || ty * SD_T < H || (tx - 1) * SD_T >= W || tx * SD_T < W) fail("tiles", H, W, ty, tx);
            for (int y0 = 0; y0 < ty * SD_T; y0 += SD_T)
                for (int x0 = 0; x0 < tx * SD_T; x0 += SD_T) {
                    const int oy0 = sd_patch_origin(y0), ox0 = sd_patch_origin(x0);
                    for (int ly = 0; ly < SD_Q; ++ly)
                        for (int lx = 0; lx < SD_Q; ++lx)
                            for (int py = 0; py < 2; ++py)
                                for (int px = 0; px < 2; ++px) {
                                    const int iy = y0 + 2 * ly + py, ix = x0 + 2 * lx + px;
                                    // the walk (also for the pixels of a ragged tile the kernel computes and does not write)
                                    uint64_t walk = 0;
                                    for (int dy = SD_DMIN; dy <= SD_DMAX; ++dy)
                                        for (int dx = SD_DMIN; dx <= SD_DMAX; ++dx) {
                                            const int ky = sd_tap_of(py, dy), kx = sd_tap_of(px, dx);
                                            if (ky < 0 || kx < 0) continue;
                                            const int hy = sd_patch_index(ly, ky), hx = sd_patch_index(lx, kx);
                                            ++touched;
                                            if (hy < 0 || hy >= SD_PATCH || hx < 0 || hx >= SD_PATCH) { fail("index outside the declared patch", H, W, hy, hx); continue; }
                                            const int oy = oy0 + hy, ox = ox0 + hx;
                                            if (2 * oy != iy + SD_PAD - ky || 2 * ox != ix + SD_PAD - kx) fail("tap reads the wrong output", H, W, oy, ox);
                                            if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) { ++outside; continue; }      // staged as zeros
                                            if (walk >> (ky * SD_K + kx) & 1) fail("tap walked twice", H, W, ky, kx);
                                            walk |= 1ull << (ky * SD_K + kx);
                                        }
                                    if (iy >= H || ix >= W) continue;
                                    ++cover[(size_t)iy * W + ix];
                                    ++pixels;
                                    // brute force per axis, and the header's own list
                                    int by[SD_K], bx[SD_K];
                                    const uint32_t my = brute_axis(iy, H, Ho, by), mx = brute_axis(ix, W, Wo, bx);
                                    uint64_t want = 0;
                                    for (int ky = 0; ky < SD_K; ++ky)
                                        for (int kx = 0; kx < SD_K; ++kx)
                                            if ((my >> ky & 1) && (mx >> kx & 1)) { want |= 1ull << (ky * SD_K + kx); ++taps; }
                                    if (walk != want) fail("tap set of a pixel", H, W, iy, ix);
                                    const SdTaps ty_ = sd_pixel_taps(iy, Ho), tx_ = sd_pixel_taps(ix, Wo);
                                    uint32_t ly_ = 0, lx_ = 0;
                                    for (int t = 0; t < ty_.n; ++t) { ly_ |= 1u << ty_.k[t]; if (ty_.o[t] != by[ty_.k[t]]) fail("tap list: output row", H, W, iy, ty_.k[t]); }
                                    for (int t = 0; t < tx_.n; ++t) { lx_ |= 1u << tx_.k[t]; if (tx_.o[t] != bx[tx_.k[t]]) fail("tap list: output column", H, W, ix, tx_.k[t]); }
                                    if (ly_ != my || lx_ != mx || ty_.n > 4 || tx_.n > 4) fail("tap list of a pixel", H, W, iy, ix);
                                }
                }
            for (size_t i = 0; i < cover.size(); ++i)
                if (cover[i] != 1) { fail("tiles do not cover every input pixel once", H, W, (long)i, cover[i]); break; }
        }
    std::printf("sweep: H, W = 1..40, tile %d, patch %d: %ld pixels, %ld taps inside the map, %ld indices walked, %ld of them outside the map\n",
                SD_T, SD_PATCH, pixels, taps, touched, outside);
    // (1 + .. + 40)^2 pixels; a quad walks 49 indices whatever its position, and some of the sweep's lie outside the map
    if (pixels != 820L * 820 || touched % 49 || taps <= 0 || taps + outside > touched || outside <= 0) fail("pinned counts", 0, 0, pixels, touched);
    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
