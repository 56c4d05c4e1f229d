// Host-only check of ust-run_amd/csrc/components.h (tests/test_components_host.py compiles this with --cuda-host-only): the helpers
// the kernels of components.hip run are driven sequentially in the kernels' order -- tile-local merges, then the border pairs, then
// flatten -- with the kernel's own tile constants, over planes built to break label merging, and compared with a flood fill written
// here.  Every forest is built twice, the unions in forward and in reverse order: the labels must not depend on the order.  The
// border-pair enumeration must name every neighbour pair across a tile edge or corner exactly once, for each connectivity.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>
#include "../../ust-run_amd/csrc/components.h"

using namespace ustrun::cc;
typedef std::vector<unsigned char> Plane;

static int failures = 0;
static long united = 0, skipped = 0;      // border pairs with both pixels members: united, left out as redundant
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the kernels' order, sequentially (local_kernel -> merge_kernel -> flatten_kernel)
static std::vector<int> forest(const Plane& m, int H, int W, int conn, bool outside, bool reverse) {
    std::vector<int> P((size_t)H * W + 1, -1);
    P[OUTSIDE] = OUTSIDE;
    for (int ty = 0; ty < tiles_y(H); ++ty)
        for (int tx = 0; tx < tiles_x(W); ++tx) {
            const int y0 = ty * TILE_H, x0 = tx * TILE_W;
            int lab[TILE_PIX], touch[TILE_PIX];
            for (int ly = 0; ly < TILE_H; ++ly) {
                unsigned long long row = 0;
                for (int lx = 0; lx < TILE_W; ++lx)
                    if (y0 + ly < H && x0 + lx < W && m[(size_t)(y0 + ly) * W + x0 + lx]) row |= 1ull << lx;
                for (int lx = 0; lx < TILE_W; ++lx) { lab[ly * TILE_W + lx] = tile_init(row, ly, lx); touch[ly * TILE_W + lx] = 0; }
            }
            for (int k = 0; k < TILE_PIX; ++k) tile_unite_pixel<Plain>(lab, reverse ? TILE_PIX - 1 - k : k, conn);
            for (int i = 0; i < TILE_PIX; ++i) {
                const int y = y0 + i / TILE_W, x = x0 + i % TILE_W;
                if (lab[i] >= 0 && (y == 0 || x == 0 || y == H - 1 || x == W - 1)) touch[find<Plain>(lab, i)] = 1;
            }
            for (int i = 0; i < TILE_PIX; ++i) {
                const int y = y0 + i / TILE_W, x = x0 + i % TILE_W;
                if (y >= H || x >= W || lab[i] < 0) continue;
                const int r = find<Plain>(lab, i);
                P[node((long)y * W + x)] = outside && touch[r] ? OUTSIDE : tile_node(r, y0, x0, W);
            }
        }
    const long slots = border_slots(conn, H, W);
    for (long k = 0; k < slots; ++k) {
        int ya, xa, yb, xb, kind, y, x;
        if (!border_pair(conn, H, W, reverse ? slots - 1 - k : k, &ya, &xa, &yb, &xb, &kind, &y, &x)) continue;
        const int a = node((long)ya * W + xa), b = node((long)yb * W + xb);
        const auto mem = [&](int v, int u) { return P[node((long)v * W + u)] >= 0; };
        if (P[a] < 0 || P[b] < 0) continue;
        if (pair_redundant(kind, y, x, W, mem)) { ++skipped; continue; }
        ++united;
        unite<Plain>(P.data(), a, b);
    }
    for (long e = 0; e < (long)H * W; ++e)
        if (P[node(e)] >= 0) P[node(e)] = find<Plain>(P.data(), node(e));
    return P;
}

// ---- the flood fill: component id per pixel (-1: not a member), ids in raster order of the first pixel; id -2 = reaches the outside
static std::vector<int> flood(const Plane& m, int H, int W, int conn, bool outside) {
    std::vector<int> id((size_t)H * W, -1);
    std::vector<std::pair<int, int>> stack;
    int next = 0;
    auto run = [&](int sy, int sx, int tag) {
        if (!m[(size_t)sy * W + sx] || id[(size_t)sy * W + sx] != -1) return false;
        id[(size_t)sy * W + sx] = tag;
        stack.push_back({sy, sx});
        while (!stack.empty()) {
            const int y = stack.back().first, x = stack.back().second;
            stack.pop_back();
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((dy == 0 && dx == 0) || (conn == 4 && dy != 0 && dx != 0)) continue;
                    const int v = y + dy, u = x + dx;
                    if (v < 0 || u < 0 || v >= H || u >= W || !m[(size_t)v * W + u] || id[(size_t)v * W + u] != -1) continue;
                    id[(size_t)v * W + u] = tag;
                    stack.push_back({v, u});
                }
        }
        return true;
    };
    if (outside)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (y == 0 || x == 0 || y == H - 1 || x == W - 1) run(y, x, -2);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (run(y, x, next)) ++next;
    return id;
}

// the forest's partition equals the flood fill's, and every root is its component's smallest node (node 0 for the outside)
static void compare(const char* what, const Plane& m, int H, int W, int conn, bool outside) {
    const std::vector<int> id = flood(m, H, W, conn, outside);
    for (int rev = 0; rev < 2; ++rev) {
        const std::vector<int> P = forest(m, H, W, conn, outside, rev);
        std::map<int, int> first;                      // flood id -> node of its first pixel in raster order
        for (long e = 0; e < (long)H * W; ++e) {
            const int r = P[node(e)];
            if (!m[e]) { EXPECT(r == -1 && id[e] == -1, "%s %dx%d conn %d: non-member %ld labelled %d", what, H, W, conn, e, r); continue; }
            if (id[e] == -2) { EXPECT(r == OUTSIDE, "%s %dx%d: pixel %ld reaches the border, root %d", what, H, W, e, r); continue; }
            if (!first.count(id[e])) first[id[e]] = node(e);
            EXPECT(r == first[id[e]], "%s %dx%d conn %d rev %d: pixel %ld root %d, flood fill says %d", what, H, W, conn, rev, e, r, first[id[e]]);
        }
    }
}

// ---- the whole post-processing of one plane, helpers against flood fill
static Plane process_helpers(const Plane& p, int H, int W, int num, int den) {
    Plane bg(p.size()), f(p.size());
    for (size_t e = 0; e < p.size(); ++e) bg[e] = !p[e];
    const std::vector<int> A = forest(bg, H, W, 4, true, false);
    long total = 0;
    for (size_t e = 0; e < p.size(); ++e) total += f[e] = p[e] || A[node(e)] > OUTSIDE;
    const std::vector<int> B = forest(f, H, W, 8, false, true);
    std::vector<int> size((size_t)H * W + 1, 0);
    for (size_t e = 0; e < p.size(); ++e) if (f[e]) ++size[B[node(e)]];
    Plane out(f);
    for (size_t e = 0; e < p.size(); ++e) if (f[e] && removed(size[B[node(e)]], total, num, den)) out[e] = 0;
    return out;
}
static Plane process_flood(const Plane& p, int H, int W) {
    Plane bg(p.size()), f(p.size());
    for (size_t e = 0; e < p.size(); ++e) bg[e] = !p[e];
    const std::vector<int> a = flood(bg, H, W, 4, true);
    long total = 0;
    for (size_t e = 0; e < p.size(); ++e) total += f[e] = p[e] || a[e] >= 0;
    const std::vector<int> b = flood(f, H, W, 8, false);
    std::map<int, long> size;
    for (size_t e = 0; e < p.size(); ++e) if (f[e]) ++size[b[e]];
    Plane out(f);
    for (size_t e = 0; e < p.size(); ++e) if (f[e] && 5 * size[b[e]] < total) out[e] = 0;      // |c| / total < 0.2
    return out;
}

// ---- planes
static unsigned rnd_state = 12345;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static std::vector<std::pair<const char*, Plane>> planes(int H, int W) {
    std::vector<std::pair<const char*, Plane>> out;
    auto blank = [&]() { return Plane((size_t)H * W, 0); };
    auto at = [&](Plane& p, int y, int x) -> unsigned char& { static unsigned char sink; return y >= 0 && x >= 0 && y < H && x < W ? p[(size_t)y * W + x] : (sink = 0, sink); };
    out.push_back({"empty", blank()});
    out.push_back({"full", Plane((size_t)H * W, 1)});
    { Plane p = blank(); for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) p[(size_t)y * W + x] = (y + x) & 1; out.push_back({"checkerboard", p}); }
    { Plane p = blank();                               // serpentine: full rows every other line, joined at alternating ends
      for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) p[(size_t)y * W + x] = y % 2 == 0 || x == ((y / 2) % 2 ? 0 : W - 1);
      out.push_back({"serpentine", p}); }
    { Plane p = blank();                               // comb: a spine along the top, teeth on every other column
      for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) p[(size_t)y * W + x] = y == 0 || x % 2 == 0;
      out.push_back({"comb", p}); }
    { Plane p = blank();                               // one-pixel-wide square spiral, walls two apart
      int y0 = 0, x0 = 0, y1 = H - 1, x1 = W - 1, y = 0, x = 0;
      while (y0 <= y1 && x0 <= x1) {
          for (x = x0; x <= x1; ++x) at(p, y0, x) = 1;
          for (y = y0; y <= y1; ++y) at(p, y, x1) = 1;
          if (y1 - y0 < 2 || x1 - x0 < 2) break;
          for (x = x1; x >= x0 + 2; --x) at(p, y1, x) = 1;
          for (y = y1; y >= y0 + 2; --y) at(p, y, x0 + 2) = 1;
          y0 += 2; x0 += 2; y1 -= 2; x1 -= 2;
          at(p, y0, x0) = 1;
          if (y1 - y0 < 2 || x1 - x0 < 2) break;
      }
      out.push_back({"spiral", p}); }
    { Plane p = blank();                               // 2x2 blocks that touch only diagonally across the tile corners, both diagonals
      for (int dy = -2; dy < 0; ++dy) for (int dx = -2; dx < 0; ++dx) { at(p, TILE_H + dy, TILE_W + dx) = 1; at(p, TILE_H + 2 + dy, TILE_W + 2 + dx) = 1; }
      for (int dy = -2; dy < 0; ++dy) for (int dx = -2; dx < 0; ++dx) { at(p, 2 * TILE_H + dy, TILE_W + 2 + dx) = 1; at(p, 2 * TILE_H + 2 + dy, TILE_W + dx) = 1; }
      at(p, TILE_H - 1, W > 8 ? 3 : 0) = 1; at(p, TILE_H, W > 8 ? 4 : 0) = 1;
      out.push_back({"corner_diagonals", p}); }
    { Plane p = blank();                               // two bars with one background column between them on the tile edge
      for (int y = 1; y < H - 1; ++y) for (int x = TILE_W - 6; x < TILE_W + 6; ++x) if (x != TILE_W) at(p, y, x) = 1;
      for (int x = 1; x < W - 1; ++x) if (x < TILE_W - 8) { at(p, TILE_H - 2, x) = 1; at(p, TILE_H, x) = 1; }
      out.push_back({"one_column_apart", p}); }
    for (int closed = 0; closed < 2; ++closed) {       // a box whose inside reaches the border through a one-pixel gap; or the gap closed diagonally
        Plane p = blank();
        const int b = std::min(H, W) - 2;
        for (int k = 1; k <= b; ++k) { at(p, 1, k) = 1; at(p, b, k) = 1; at(p, k, 1) = 1; at(p, k, b) = 1; }
        at(p, 1, b / 2) = 0;                           // the gap: the inside leaks through it to row 0
        if (closed) {                                  // row 0 filled but for the pixel diagonally above the gap: no 4-path left
            for (int x = 0; x < W; ++x) at(p, 0, x) = 1;
            at(p, 0, b / 2 + 1) = 0;
        }
        out.push_back({closed ? "gap_closed" : "gap_open", p});
    }
    { Plane p = blank();                               // nested rings
      const int cy = H / 2, cx = W / 2;
      for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) { const int d = std::max(abs(y - cy), abs(x - cx)); p[(size_t)y * W + x] = d % 4 == 1 && d < std::min(H, W) / 2; }
      out.push_back({"nested_rings", p}); }
    { Plane p = blank();                               // the 1/5 boundary: five 2x2 squares, then one more pixel
      for (int k = 0; k < 5; ++k) for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx) at(p, 1 + dy, 1 + 3 * k + dx) = 1;
      out.push_back({"five_squares", p});
      at(p, H - 1, W - 1) = 1;
      out.push_back({"five_squares_plus_one", p}); }
    static const int flips[3] = {0, 2, 30};
    for (int f = 0; f < 3; ++f) {
        Plane p = blank();
        for (int k = 0; k < 3; ++k) {
            const int cy = rnd() % H, cx = rnd() % W, r = 2 + rnd() % (std::max(H, W) / 3 + 1);
            for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) if ((y - cy) * (y - cy) + (x - cx) * (x - cx) <= r * r && (y - cy) * (y - cy) + (x - cx) * (x - cx) >= (r / 2) * (r / 2)) p[(size_t)y * W + x] = 1;
        }
        for (size_t e = 0; e < p.size(); ++e) if ((int)(rnd() % 100) < flips[f]) p[e] ^= 1;
        out.push_back({f == 0 ? "blobs" : f == 1 ? "blobs_2pc" : "blobs_30pc", p});
    }
    return out;
}

// every neighbour pair whose pixels lie in different tiles is named by exactly one slot
static void check_border_pairs(int conn, int H, int W) {
    std::map<std::pair<int, int>, int> want;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < fwd_count(conn); ++k) {
                int dy, dx;
                fwd_offset(k, &dy, &dx);
                const int v = y + dy, u = x + dx;
                if (v < 0 || u < 0 || u >= W) continue;
                if (y / TILE_H == v / TILE_H && x / TILE_W == u / TILE_W) continue;
                want[{std::min(y * W + x, v * W + u), std::max(y * W + x, v * W + u)}] = 0;
            }
    const long slots = border_slots(conn, H, W);
    for (long s = 0; s < slots; ++s) {
        int ya, xa, yb, xb;
        if (!border_pair(conn, H, W, s, &ya, &xa, &yb, &xb)) continue;
        EXPECT(ya >= 0 && ya < H && yb >= 0 && yb < H && xa >= 0 && xa < W && xb >= 0 && xb < W, "pair out of the image: %dx%d conn %d slot %ld", H, W, conn, s);
        const int a = ya * W + xa, b = yb * W + xb;
        auto it = want.find({std::min(a, b), std::max(a, b)});
        EXPECT(it != want.end(), "%dx%d conn %d slot %ld names (%d,%d)-(%d,%d), which crosses no tile edge or is no neighbour pair", H, W, conn, s, ya, xa, yb, xb);
        if (it != want.end()) ++it->second;
    }
    for (auto& kv : want) EXPECT(kv.second == 1, "%dx%d conn %d: pair %d-%d named %d times", H, W, conn, kv.first.first, kv.first.second, kv.second);
}

int main() {
    static const int sizes[][2] = {{1, 1}, {1, 37}, {37, 1}, {16, 16}, {17, 23}, {33, 65}, {64, 64}, {96, 136}, {130, 70},
                                   {TILE_H, TILE_W}, {TILE_H + 1, TILE_W + 1}, {2 * TILE_H, 2 * TILE_W}, {3 * TILE_H - 1, 3 * TILE_W - 1}};
    int nplanes = 0;
    for (auto& hw : sizes) {
        const int H = hw[0], W = hw[1];
        for (int conn = 4; conn <= 8; conn += 4) check_border_pairs(conn, H, W);
        for (auto& np : planes(H, W)) {
            const Plane& p = np.second;
            Plane bg(p.size());
            for (size_t e = 0; e < p.size(); ++e) bg[e] = !p[e];
            compare(np.first, bg, H, W, 4, true);          // the hole search
            compare(np.first, p, H, W, 8, false);          // the components
            compare(np.first, p, H, W, 4, false);
            const Plane got = process_helpers(p, H, W, 1, 5), want = process_flood(p, H, W);
            EXPECT(got == want, "%s %dx%d: post-processing differs from the flood fill's", np.first, H, W);
            ++nplanes;
        }
    }
    EXPECT(!removed(4, 20, 1, 5) && removed(4, 21, 1, 5) && !removed(1, 1 << 20, 0, 1) && removed((1 << 20) - 1, 1 << 20, 1, 1), "filter predicate");
    EXPECT(removed(1LL << 19, 1LL << 20, 2000000000, 2000000000 / 2 - 1), "filter predicate: 64-bit products");
    EXPECT(united > 0 && skipped > united, "border pairs: %ld united, %ld redundant", united, skipped);
    printf("border pairs between members: %ld united, %ld left out as redundant\n", united, skipped);
    printf("tile %d x %d, %d planes over %d sizes\n", TILE_H, TILE_W, nplanes, (int)(sizeof(sizes) / sizeof(sizes[0])));
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
