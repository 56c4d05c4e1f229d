// Host-only check of ust-run_amd/csrc/components3d.h beside components.h (tests/test_components3d_host.py compiles this with
// --cuda-host-only): the helpers the kernels of components3d.hip run are driven sequentially in the kernels' order -- slice-local
// tile merges, the in-plane border pairs, the pairs between adjacent slices with their redundancy rules, flatten -- with the kernel's
// own constants, over volumes built to break label merging, and compared with a flood fill written here.  Every forest is built with
// the unions in forward and in reverse order, and with the redundant z-pairs left out and united: the labels must not depend on
// either.  The z-pair enumeration must name every neighbour pair between adjacent slices exactly once, for fan 1 and fan 9.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <utility>
#include <vector>
#include "../../ust-run_amd/csrc/components3d.h"

using namespace ustrun::cc;
typedef std::vector<unsigned char> Vol;

static int failures = 0;
static long united = 0, skipped = 0;      // z-pairs with both voxels members: united, left out as redundant
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the kernels' order, sequentially (local_kernel -> merge_kernel -> zmerge_kernel -> flatten_kernel).  conn 4: the hole search
// (cross in the slice, fan 1 between slices, node 0 for what touches a face); conn 8: the components (3 x 3 square, fan 9).
static std::vector<int> forest(const Vol& m, int D, int H, int W, int conn, bool outside, bool reverse, bool prune) {
    const int HW = H * W, fan = conn == 8 ? 9 : 1;
    std::vector<int> P((size_t)D * HW + 1, -1);
    P[OUTSIDE] = OUTSIDE;
    for (int z = 0; z < D; ++z)
        for (int ty = 0; ty < tiles_y(H); ++ty)
            for (int tx = 0; tx < tiles_x(W); ++tx) {
                const int y0 = ty * TILE_H, x0 = tx * TILE_W, zoff = z * HW;
                int lab[TILE_PIX], touch[TILE_PIX];
                for (int ly = 0; ly < TILE_H; ++ly) {
                    unsigned long long row = 0;
                    for (int lx = 0; lx < TILE_W; ++lx)
                        if (y0 + ly < H && x0 + lx < W && m[(size_t)zoff + (y0 + ly) * W + x0 + lx]) row |= 1ull << lx;
                    for (int lx = 0; lx < TILE_W; ++lx) { lab[ly * TILE_W + lx] = tile_init(row, ly, lx); touch[ly * TILE_W + lx] = 0; }
                }
                for (int k = 0; k < TILE_PIX; ++k) tile_unite_pixel<Plain>(lab, reverse ? TILE_PIX - 1 - k : k, conn);
                for (int i = 0; i < TILE_PIX; ++i)
                    if (lab[i] >= 0 && on_face(z, y0 + i / TILE_W, x0 + i % TILE_W, D, H, W)) touch[find<Plain>(lab, i)] = 1;
                for (int i = 0; i < TILE_PIX; ++i) {
                    const int y = y0 + i / TILE_W, x = x0 + i % TILE_W;
                    if (y >= H || x >= W || lab[i] < 0) continue;
                    const int r = find<Plain>(lab, i);
                    P[vnode(z, y, x, H, W)] = outside && touch[r] ? OUTSIDE : zoff + tile_node(r, y0, x0, W);
                }
            }
    const long slots = border_slots(conn, H, W);
    for (long k = 0; k < slots * D; ++k) {
        const long idx = reverse ? slots * D - 1 - k : k;
        const int zoff = (int)(idx / slots) * HW;
        int ya, xa, yb, xb, kind, y, x;
        if (!border_pair(conn, H, W, idx % slots, &ya, &xa, &yb, &xb, &kind, &y, &x)) continue;
        const int a = zoff + node((long)ya * W + xa), b = zoff + node((long)yb * W + xb);
        const auto mem = [&](int v, int u) { return P[zoff + node((long)v * W + u)] >= 0; };
        if (P[a] < 0 || P[b] < 0 || pair_redundant(kind, y, x, W, mem)) continue;
        unite<Plain>(P.data(), a, b);
    }
    const long zs = z_slots(fan, D, H, W);
    for (long k = 0; k < zs; ++k) {
        int z, y, x, dy, dx;
        if (!z_pair(fan, H, W, reverse ? zs - 1 - k : k, &z, &y, &x, &dy, &dx)) continue;
        const auto mem = [&](int w, int v, int u) { return P[vnode(w, v, u, H, W)] >= 0; };
        if (!mem(z, y, x) || !mem(z - 1, y + dy, x + dx)) continue;
        if (prune && z_pair_redundant(z, y, x, dy, dx, mem)) { ++skipped; continue; }
        united += prune;
        unite<Plain>(P.data(), vnode(z, y, x, H, W), vnode(z - 1, y + dy, x + dx, H, W));
    }
    for (long e = 0; e < (long)D * HW; ++e)
        if (P[node(e)] >= 0) P[node(e)] = find<Plain>(P.data(), node(e));
    return P;
}

// ---- the flood fill: component id per voxel (-1: not a member), ids in raster order of the first voxel; id -2 = reaches the outside.
// conn 4 stands for the 6 face neighbours, conn 8 for all 26.
static std::vector<int> flood(const Vol& m, int D, int H, int W, int conn, bool outside) {
    std::vector<int> id(m.size(), -1);
    std::vector<int> stack;
    int next = 0;
    auto run = [&](int s, int tag) {
        if (!m[s] || id[s] != -1) return false;
        id[s] = tag;
        stack.push_back(s);
        while (!stack.empty()) {
            const int e = stack.back(), z = e / (H * W), y = e / W % H, x = e % W;
            stack.pop_back();
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int n = abs(dz) + abs(dy) + abs(dx);
                        if (n == 0 || (conn == 4 && n != 1)) continue;
                        const int w = z + dz, v = y + dy, u = x + dx;
                        if (w < 0 || v < 0 || u < 0 || w >= D || v >= H || u >= W) continue;
                        const int q = (w * H + v) * W + u;
                        if (!m[q] || id[q] != -1) continue;
                        id[q] = tag;
                        stack.push_back(q);
                    }
        }
        return true;
    };
    if (outside)
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (on_face(z, y, x, D, H, W)) run((z * H + y) * W + x, -2);
    for (int e = 0; e < (int)m.size(); ++e)
        if (run(e, next)) ++next;
    return id;
}

// the forest's partition equals the flood fill's, and every root is its component's smallest node (node 0 for the outside)
static void compare(const char* what, const Vol& m, int D, int H, int W, int conn, bool outside) {
    const std::vector<int> id = flood(m, D, H, W, conn, outside);
    for (int variant = 0; variant < 4; ++variant) {
        const bool rev = variant & 1, prune = !(variant & 2);
        const std::vector<int> P = forest(m, D, H, W, conn, outside, rev, prune);
        std::map<int, int> first;                      // flood id -> node of its first voxel in raster order
        for (long e = 0; e < (long)m.size(); ++e) {
            const int r = P[node(e)];
            if (!m[e]) { EXPECT(r == -1 && id[e] == -1, "%s %dx%dx%d conn %d: non-member %ld labelled %d", what, D, H, W, conn, e, r); continue; }
            if (id[e] == -2) { EXPECT(r == OUTSIDE, "%s %dx%dx%d rev %d prune %d: voxel %ld reaches a face, root %d", what, D, H, W, rev, prune, e, r); continue; }
            if (!first.count(id[e])) first[id[e]] = node(e);
            EXPECT(r == first[id[e]], "%s %dx%dx%d conn %d rev %d prune %d: voxel %ld root %d, flood fill says %d", what, D, H, W, conn, rev, prune, e, r, first[id[e]]);
        }
    }
}

// ---- the whole post-processing of one volume, helpers against flood fill
static Vol process_helpers(const Vol& p, int D, int H, int W, int num, int den, bool largest) {
    Vol bg(p.size()), f(p.size());
    for (size_t e = 0; e < p.size(); ++e) bg[e] = !p[e];
    const std::vector<int> A = forest(bg, D, H, W, 4, true, false, true);
    long total = 0;
    for (size_t e = 0; e < p.size(); ++e) total += f[e] = p[e] || A[node(e)] > OUTSIDE;
    const std::vector<int> B = forest(f, D, H, W, 8, false, true, true);
    std::vector<int> size(p.size() + 1, 0);
    for (size_t e = 0; e < p.size(); ++e) if (f[e]) ++size[B[node(e)]];
    unsigned long long key = 0;
    for (size_t e = 0; e < p.size(); ++e) if (f[e] && B[node(e)] == node(e)) key = std::max(key, largest_key(size[node(e)], node(e)));
    Vol out(f);
    for (size_t e = 0; e < p.size(); ++e)
        if (f[e] && (removed(size[B[node(e)]], total, num, den) || (largest && B[node(e)] != key_root(key)))) out[e] = 0;
    return out;
}
static Vol process_flood(const Vol& p, int D, int H, int W, int num, int den, bool largest) {
    Vol bg(p.size()), f(p.size());
    for (size_t e = 0; e < p.size(); ++e) bg[e] = !p[e];
    const std::vector<int> a = flood(bg, D, H, W, 4, true);
    long total = 0;
    for (size_t e = 0; e < p.size(); ++e) total += f[e] = p[e] || a[e] >= 0;
    const std::vector<int> b = flood(f, D, H, W, 8, false);
    std::map<int, long> size;
    for (size_t e = 0; e < p.size(); ++e) if (f[e]) ++size[b[e]];
    int best = -1;                                     // ids are in raster order of the first voxel: the first of the largest wins
    for (auto& kv : size) if (best < 0 || kv.second > size[best]) best = kv.first;
    Vol out(f);
    for (size_t e = 0; e < p.size(); ++e)
        if (f[e] && ((long long)den * size[b[e]] < (long long)num * total || (largest && b[e] != best))) out[e] = 0;
    return out;
}

// ---- volumes
static unsigned rnd_state = 22222;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static std::vector<std::pair<const char*, Vol>> volumes(int D, int H, int W) {
    std::vector<std::pair<const char*, Vol>> out;
    auto blank = [&]() { return Vol((size_t)D * H * W, 0); };
    auto at = [&](Vol& p, int z, int y, int x) -> unsigned char& {
        static unsigned char sink;
        return z >= 0 && y >= 0 && x >= 0 && z < D && y < H && x < W ? p[((size_t)z * H + y) * W + x] : (sink = 0, sink);
    };
    out.push_back({"empty", blank()});
    out.push_back({"full", Vol((size_t)D * H * W, 1)});
    static const int dens[3] = {15, 30, 50};
    for (int k = 0; k < 3; ++k) {
        Vol p = blank();
        for (size_t e = 0; e < p.size(); ++e) p[e] = (int)(rnd() % 100) < dens[k];
        out.push_back({k == 0 ? "random_15" : k == 1 ? "random_30" : "random_50", p});
    }
    { Vol p = blank(); for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) at(p, z, y, x) = (z + y + x) & 1; out.push_back({"checkerboard", p}); }
    for (int axis = 0; axis < 3; ++axis) {             // a tube along each axis: a ring in every cross-section, open at both ends
        Vol p = blank();
        for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
            const int a = axis == 0 ? y : z, b = axis == 2 ? y : x, A = axis == 0 ? H : D, B = axis == 2 ? H : W;
            const bool ring = a >= 1 && b >= 1 && a <= A - 2 && b <= B - 2 && (a == 1 || b == 1 || a == A - 2 || b == B - 2);
            at(p, z, y, x) = ring;
        }
        out.push_back({axis == 0 ? "tube_z" : axis == 1 ? "tube_y" : "tube_x", p});
    }
    { Vol p = blank();                                 // nested closed shells: Chebyshev distance from the centre 1 mod 2... every other layer
      for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
          const int d = std::min({z, y, x, D - 1 - z, H - 1 - y, W - 1 - x});
          at(p, z, y, x) = d % 2 == 1;
      }
      out.push_back({"nested_shells", p}); }
    { Vol p = blank();                                 // closed box around the whole interior
      for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) at(p, z, y, x) = on_face(z, y, x, D, H, W);
      if (D > 2 && H > 2 && W > 2) at(p, D / 2, H / 2, W / 2) = 1;
      out.push_back({"closed_box", p}); }
    { Vol p = blank();                                 // 3-D serpentine: the plane serpentine in every other slice, slices joined at alternating corners
      for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
          if (z % 2 == 0) at(p, z, y, x) = y % 2 == 0 || x == ((y / 2) % 2 ? 0 : W - 1);
          else at(p, z, y, x) = ((z / 2) % 2 ? (y == 0 && x == 0) : (y == H - 1 && x == W - 1));
      }
      out.push_back({"serpentine", p}); }
    { Vol p = blank();                                 // a spiral through the slices: one row per slice, the row moving round, joined by corners only
      for (int z = 0; z < D; ++z) { const int y = (z * 3) % H; for (int x = z % 2; x < W; x += 1) at(p, z, y, x) = (x / 3 + z) % 2 == 0; at(p, z, (y + 1) % H, (z * 7) % W) = 1; }
      out.push_back({"spiral", p}); }
    { Vol p = blank();                                 // voxels that touch only by a corner across a tile corner and a slice
      for (int z = 0; z < D; ++z) {
          at(p, z, TILE_H - 1 + (z & 1), TILE_W - 1 + (z & 1)) = 1;
          at(p, z, TILE_H - (z & 1), TILE_W - 1 + (z & 1)) = 1;
          at(p, z, 1 + (z & 1), 1 + (z & 1)) = 1;
      }
      at(p, D - 1, H - 1, W - 1) = 1;
      out.push_back({"corner_touch", p}); }
    { Vol p = blank();                                 // the 1/5 boundary: five 2x2 squares, then one more voxel
      for (int k = 0; k < 5; ++k) for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx) at(p, 0, 1 + dy, 1 + 3 * k + dx) = 1;
      out.push_back({"five_squares", p});
      at(p, D - 1, H - 1, W - 1) = 1;
      out.push_back({"five_squares_plus_one", p}); }
    return out;
}

// every neighbour pair between adjacent slices is named by exactly one slot
static void check_z_pairs(int fan, int D, int H, int W) {
    std::map<std::pair<int, int>, int> want;
    for (int z = 1; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (fan == 1 && (dy || dx)) continue;
                        const int v = y + dy, u = x + dx;
                        if (v < 0 || u < 0 || v >= H || u >= W) continue;
                        want[{((z - 1) * H + v) * W + u, (z * H + y) * W + x}] = 0;
                    }
    const long slots = z_slots(fan, D, H, W);
    EXPECT(slots == (long)fan * (D - 1) * H * W, "z_slots");
    for (long s = 0; s < slots; ++s) {
        int z, y, x, dy, dx;
        if (!z_pair(fan, H, W, s, &z, &y, &x, &dy, &dx)) continue;
        EXPECT(z >= 1 && z < D && y >= 0 && y < H && x >= 0 && x < W && y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W,
               "pair out of the volume: %dx%dx%d fan %d slot %ld", D, H, W, fan, s);
        auto it = want.find({((z - 1) * H + y + dy) * W + x + dx, (z * H + y) * W + x});
        EXPECT(it != want.end(), "%dx%dx%d fan %d slot %ld names no neighbour pair", D, H, W, fan, s);
        if (it != want.end()) ++it->second;
    }
    for (auto& kv : want) EXPECT(kv.second == 1, "%dx%dx%d fan %d: pair %d-%d named %d times", D, H, W, fan, kv.first.first, kv.first.second, kv.second);
}

int main() {
    static const int sizes[][3] = {{1, 1, 1}, {1, 5, 5}, {2, 17, 65}, {3, 16, 64}, {5, 19, 70}, {7, 3, 5}, {4, 33, 130}, {9, 1, 7}, {6, 7, 1},
                                   {3, TILE_H + 1, 2 * TILE_W}};
    int nvol = 0;
    for (auto& s : sizes) {
        const int D = s[0], H = s[1], W = s[2];
        check_z_pairs(1, D, H, W);
        check_z_pairs(9, D, H, W);
        for (auto& nv : volumes(D, H, W)) {
            const Vol& p = nv.second;
            Vol bg(p.size());
            for (size_t e = 0; e < p.size(); ++e) bg[e] = !p[e];
            compare(nv.first, bg, D, H, W, 4, true);           // the hole search
            compare(nv.first, p, D, H, W, 8, false);           // the components
            compare(nv.first, p, D, H, W, 4, false);
            static const int shares[][2] = {{1, 5}, {1, 2}, {1, 1}, {0, 1}};
            for (auto& sh : shares)
                for (int largest = 0; largest < 2; ++largest) {
                    const Vol got = process_helpers(p, D, H, W, sh[0], sh[1], largest), want = process_flood(p, D, H, W, sh[0], sh[1], largest);
                    EXPECT(got == want, "%s %dx%dx%d share %d/%d largest %d: post-processing differs from the flood fill's", nv.first, D, H, W, sh[0], sh[1], largest);
                }
            ++nvol;
        }
    }
    EXPECT(largest_key(5, 3) > largest_key(5, 4) && largest_key(6, 9) > largest_key(5, 1) && key_root(largest_key(1 << 27, (1 << 27))) == (1 << 27) && key_root(0) < 0,
           "largest key");
    EXPECT(united > 0 && skipped > united, "z-pairs: %ld united, %ld redundant", united, skipped);
    printf("z-pairs between members: %ld united, %ld left out as redundant\n", united, skipped);
    printf("tile %d x %d, %d volumes over %d sizes\n", TILE_H, TILE_W, nvol, (int)(sizeof(sizes) / sizeof(sizes[0])));
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
