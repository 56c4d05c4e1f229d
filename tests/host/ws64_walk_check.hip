// ws64_walk_check.hip -- host-only check of the plan and the cursor of the 64 -> 64 streaming convolution (ust-run_amd/csrc/ws64_walk.h)
// over whole ranges of shapes (tests/test_ws64_walk_host.py builds and runs it; no GPU, no device code is called).
// Exit status 0 = every check passed.
#include <cstdio>
#include <vector>
#include "../../ust-run_amd/csrc/ws64_walk.h"

using namespace ustrun;

static long g_fail = 0;
static void fail(const char* what, int N, int H, int W, long a, long b) {
    if (g_fail++ < 20) std::printf("FAIL %s (N = %d, %d x %d): %ld, %ld\n", what, N, H, W, a, b);
}
static bool same(const Cur& a, const Cur& b) {
    return a.valid == b.valid && a.item == b.item && a.img == b.img && a.x0 == b.x0 && a.ybeg == b.ybeg && a.S == b.S && a.k == b.k && a.left == b.left;
}

static const int Ws[] = {32, 80, 104, 128, 256}, Hs[] = {16, 64, 70, 72, 88, 128, 256};

// invariants of either plan
static void check_plan(const WsPlan& p, int N, int H, int W, bool keep_uniform) {
    const int steps = cdiv(H, 8);
    if (ws_grid(N, p) > 65536 || ws_grid(N, p) < 1) fail("grid", N, H, W, ws_grid(N, p), 65536);
    if (p.steps != steps || p.sx != cdiv(W, WS_TW)) fail("steps / sx", N, H, W, p.steps, p.sx);
    if (p.seg % 8 || (long)(p.sy - 1) * p.seg >= H || (long)p.sy * p.seg < H) fail("empty segment", N, H, W, p.sy, p.seg);
    if (p.items != N * p.sx * p.sy || (long)p.ipb * 256 < p.items) fail("items / ipb", N, H, W, p.items, p.ipb);
    if (keep_uniform && p.L != 0) fail("keep_uniform", N, H, W, p.L, 0);
    if (p.L > 0 && p.L < steps) fail("L >= steps", N, H, W, p.L, steps);
}

// uniform plan: every block's walk against fresh division-based decodes; the segments of a strip tile [0, H)
static long check_uniform(int N, int H, int W, std::vector<int>& cover) {
    const WsPlan p = ws_plan(N, H, W, false, false);
    check_plan(p, N, H, W, false);
    if (p.L != 0) fail("flat plan outside the consumer / producer build", N, H, W, p.L, 0);
    cover.assign((size_t)N * p.sx * H, 0);
    long groups = 0;
    const int grid = ws_grid(N, p);
    for (int b = 0; b < grid; ++b) {
        const int it0 = b * p.ipb, it1 = min(it0 + p.ipb, p.items);
        Cur c = ws_decode(p, N, H, b, it1, it0, 0, false);
        for (int item = it0; item < it1; ++item) {
            const Cur f0 = ws_decode(p, N, H, b, it1, item, 0, false);
            const int rows = min(p.seg, H - f0.ybeg);
            if (!f0.valid || f0.item != item || rows <= 0 || f0.S != (rows + 7) / 8 || f0.img < 0 || f0.img >= N || f0.x0 % WS_TW || f0.x0 >= p.sx * WS_TW
                || f0.ybeg % p.seg) { fail("uniform decode", N, H, W, item, f0.S); continue; }
            for (int y = f0.ybeg; y < f0.ybeg + rows; ++y) ++cover[((size_t)f0.img * p.sx + f0.x0 / WS_TW) * H + y];
            for (int k = 0; k <= f0.S; ++k) {
                if (!same(c, ws_decode(p, N, H, b, it1, item, k, false))) fail("uniform advance != decode", N, H, W, item, k);
                c = ws_advance(p, H, it1, c, false);
                ++groups;
            }
        }
        for (int r = 0; r < 3; ++r) {
            if (c.valid) fail("uniform walk does not end", N, H, W, b, c.item);
            c = ws_advance(p, H, it1, c, false);
        }
    }
    if (ws_decode(p, N, H, grid, min(grid * p.ipb + p.ipb, p.items), grid * p.ipb, 0, false).valid) fail("uniform: block after the last", N, H, W, grid, 0);
    for (size_t i = 0; i < cover.size(); ++i)
        if (cover[i] != 1) { fail("uniform segments do not tile the strip", N, H, W, (long)i, cover[i]); break; }
    return groups;
}

// flat plan: every (strip, step) once, a block's pieces consecutive, the item slots
static long check_flat(const WsPlan& p, int N, int H, int W, std::vector<int>& cover, std::vector<char>& slot) {
    const int total = N * p.sx * p.steps, grid = ws_grid(N, p), stat_rows = ws_stat_rows(N, p);
    cover.assign((size_t)total, 0);
    slot.assign((size_t)N * p.sx * 2, 0);
    if (stat_rows != N * p.sx * 4) fail("flat statistics rows", N, H, W, stat_rows, N * p.sx * 4);
    long pieces = 0;
    for (int b = 0; b < grid; ++b) {
        Cur c = ws_decode(p, N, H, b, 0, 0, 0, true);
        int pos = b * p.L;                   // where the next piece has to start
        const int want = min(p.L, total - pos);
        if (!c.valid) fail("flat: block without work", N, H, W, b, grid);
        while (c.valid) {
            const int strip = c.img * p.sx + c.x0 / WS_TW, st = c.ybeg / 8;
            if (c.k != 0 || c.S < 1 || c.ybeg % 8 || c.x0 % WS_TW || c.x0 >= p.sx * WS_TW || c.img >= N || st + c.S > p.steps) { fail("flat piece", N, H, W, b, c.S); break; }
            if (strip * p.steps + st != pos) fail("flat: pieces not consecutive", N, H, W, strip * p.steps + st, pos);
            if (c.item != 2 * strip + (c.ybeg != 0)) fail("flat item slot", N, H, W, c.item, 2 * strip + (c.ybeg != 0));
            if (c.item < 0 || c.item >= (int)slot.size() || slot[c.item]++) { fail("flat: item slot taken twice", N, H, W, c.item, b); break; }
            if (2 * c.item + 1 >= stat_rows) fail("flat: statistics row beyond the buffer", N, H, W, c.item, stat_rows);
            for (int s = 0; s < c.S; ++s) ++cover[(size_t)pos + s];
            pos += c.S;
            if (c.left != b * p.L + want - pos) fail("flat: steps left", N, H, W, c.left, b * p.L + want - pos);
            const Cur first = c;
            for (int k = 0; k <= first.S; ++k) {        // the piece's groups: k counts up, nothing else moves
                Cur e = first; e.k = k;
                if (!same(c, e)) fail("flat: group of a piece", N, H, W, c.item, k);
                c = ws_advance(p, H, 0, c, true);
            }
            ++pieces;
        }
        if (pos != b * p.L + want) fail("flat: block's step count", N, H, W, pos - b * p.L, want);
        for (int r = 0; r < 3; ++r) {
            c = ws_advance(p, H, 0, c, true);
            if (c.valid) fail("flat walk does not end", N, H, W, b, c.item);
        }
    }
    if (ws_decode(p, N, H, grid, 0, 0, 0, true).valid) fail("flat: block after the last", N, H, W, grid, 0);
    for (size_t i = 0; i < cover.size(); ++i)
        if (cover[i] != 1) { fail("flat: step not covered exactly once", N, H, W, (long)i, cover[i]); break; }
    return pieces;
}

static void expect_L(int N, int H, int W, int L) {
    const WsPlan p = ws_plan(N, H, W, true, false);
    if (p.L != L) fail("flat plan of a pinned shape", N, H, W, p.L, L);
}

int main() {
    std::vector<int> cover;
    std::vector<char> slot;

    long shapes = 0, groups = 0;
    for (int N = 1; N <= 40; ++N)
        for (int W : Ws)
            for (int H : Hs) { groups += check_uniform(N, H, W, cover); ++shapes; }
    std::printf("uniform plan: N = 1..40 x 5 widths x 7 heights, %ld shapes, %ld groups\n", shapes, groups);

    long flat = 0, pieces = 0, pairs = 0;
    for (int N = 1; N <= 300; ++N)
        for (int W : Ws)
            for (int H : Hs) {
                const WsPlan p = ws_plan(N, H, W, true, false);
                check_plan(p, N, H, W, false);
                check_plan(ws_plan(N, H, W, true, true), N, H, W, true);
                check_plan(ws_plan(N, H, W, false, false), N, H, W, true);         // (not the consumer / producer build: uniform too)
                pairs += 3;
                if (p.L > 0) { pieces += check_flat(p, N, H, W, cover, slot); ++flat; }
            }
    expect_L(130, 64, 64, 9); expect_L(90, 70, 80, 10); expect_L(81, 256, 256, 81);
    const int pinned[2][3] = {{130, 64, 64}, {90, 70, 80}};                 // (the exact GPU cases; a width of 64 is not in the sweep)
    for (const int* s : {pinned[0], pinned[1]}) {
        const WsPlan p = ws_plan(s[0], s[1], s[2], true, false);
        check_plan(p, s[0], s[1], s[2], false);
        if (p.L > 0) { pieces += check_flat(p, s[0], s[1], s[2], cover, slot); ++flat; }
        check_uniform(s[0], s[1], s[2], cover);
    }
    std::printf("flat plan: N = 1..300 x 5 widths x 7 heights + 2 pinned shapes, %ld took the flat plan, %ld pieces\n", flat, pieces);
    std::printf("plan invariants: %ld (shape, plan) pairs\n", pairs);

    if (g_fail) { std::printf("%ld checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
