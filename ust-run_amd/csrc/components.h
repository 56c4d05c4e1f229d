// Connected-component labelling by label equivalence (components.hip: ustrun_post_process), the part that host and device share:
// the union-find steps, the neighbour rule of each connectivity, the tiles, the enumeration of the neighbour pairs that cross a
// tile edge, and the size filter.  Everything is __host__ __device__ and takes its memory accesses from a policy type, so the
// kernels' order (tile-local merges, border pairs, flatten) can be replayed sequentially on the CPU (tests/host/components_check.hip).
//
// A plane's pixel e = y * W + x is node e + 1 of a forest P[0 .. H*W]; node 0 is the virtual "outside" every background pixel of
// the image border joins when holes are searched.  P[i] is the parent, P[i] <= i always, P[i] == i at a root, and P[i] == -1 at a
// pixel that is not a member of the set being labelled (never climbed, never united).  Parents only decrease, so a `find` only
// climbs towards smaller indices and every loop below ends on any input; the component's root is its smallest node, whatever the
// order of the unions: the result does not depend on scheduling.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CC_HD inline
#endif

namespace ustrun {
namespace cc {

constexpr int TILE_H = 16, TILE_W = 64;            // one block labels one tile in LDS: 1024 pixels, one wave per row
constexpr int TILE_PIX = TILE_H * TILE_W;
constexpr int OUTSIDE = 0;

// sequential access policy (the CPU replay, and LDS or global memory no other thread is writing)
struct Plain {
    static CC_HD int load(const int* p) { return *p; }
    static CC_HD int lower(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
};

CC_HD int node(long e) { return (int)e + 1; }
CC_HD int tiles_y(int H) { return (H + TILE_H - 1) / TILE_H; }
CC_HD int tiles_x(int W) { return (W + TILE_W - 1) / TILE_W; }

// The root of i.  Every value read was i's ancestor at some time (a stale read is an older ancestor: sets only grow), and each
// step goes to a strictly smaller index: at most i steps.
template <class A>
CC_HD int find(const int* P, int i) {
    for (;;) {
        const int p = A::load(P + i);
        if (p >= i || p < 0) return i;
        i = p;
    }
}

// Joins the sets of a and b: the larger root is hung below the smaller one with A::lower (an atomic minimum on the device), which
// returns what the parent was.  If that was no longer the root itself, another union got there first: the parent is now
// min(old, b) and the set `old` leads to still has to meet b, so the step repeats with (old, b), old < a.  a + b falls every round.
template <class A>
CC_HD void unite(int* P, int a, int b) {
    for (;;) {
        a = find<A>(P, a);
        b = find<A>(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = A::lower(P + a, b);
        if (old >= a) return;
        a = old;
    }
}

// Neighbour rule.  conn 4: the cross (holes: scipy.ndimage.binary_fill_holes' default structure); conn 8: the full 3x3 square
// (skimage.measure.label's default for a plane).  Each undirected pair is named once, from its later pixel in raster order:
// the "forward" offsets k = 0 .. fwd_count - 1 are left, up, and for conn 8 up-left, up-right.
CC_HD int fwd_count(int conn) { return conn == 8 ? 4 : 2; }
CC_HD void fwd_offset(int k, int* dy, int* dx) {
    *dy = k == 0 ? 0 : -1;
    *dx = k == 0 ? -1 : k == 1 ? 0 : k == 2 ? -1 : 1;
}

// ---- neighbour pairs across tile edges and corners.  slot in [0, border_slots): first the horizontal edges (row y = r * TILE_H,
// r >= 1: pixel (y, x) with (y - 1, x + d), d = 0, or -1 / 0 / +1 for conn 8 -- corner crossings included), then the vertical
// edges (column x = c * TILE_W, c >= 1: (y, x) with (y, x - 1), and for conn 8 the two diagonals (y, x) - (y - 1, x - 1) and
// (y, x - 1) - (y - 1, x), both only where y is not a tile's first row: there the horizontal edges have them already).
CC_HD int border_fan(int conn) { return conn == 8 ? 3 : 1; }
CC_HD long border_slots(int conn, int H, int W) {
    return (long)border_fan(conn) * ((long)(tiles_y(H) - 1) * W + (long)(tiles_x(W) - 1) * H);
}
// false: the slot names no pair (a neighbour outside the image, or a diagonal the other edge kind owns).  kind and (*y, *x), the
// pixel below / right of the edge, are what pair_redundant takes: 0 1 2 = horizontal edge, upper neighbour x + 0 / - 1 / + 1;
// 3 4 5 = vertical edge: (y, x) - (y, x - 1), (y, x) - (y - 1, x - 1), (y, x - 1) - (y - 1, x)
CC_HD bool border_pair(int conn, int H, int W, long slot, int* ya, int* xa, int* yb, int* xb, int* kind, int* y, int* x) {
    const int fan = border_fan(conn);
    const long nh = (long)fan * (tiles_y(H) - 1) * W;
    if (slot < nh) {
        const int d = conn == 8 ? (int)(slot % fan) - 1 : 0;
        const long q = slot / fan;
        *y = ((int)(q / W) + 1) * TILE_H; *x = (int)(q % W);
        *kind = d == 0 ? 0 : d < 0 ? 1 : 2;
        if (*x + d < 0 || *x + d >= W) return false;
        *ya = *y; *xa = *x; *yb = *y - 1; *xb = *x + d;
        return true;
    }
    slot -= nh;
    const int k = (int)(slot % fan);
    const long q = slot / fan;
    *x = ((int)(q / H) + 1) * TILE_W; *y = (int)(q % H);
    *kind = 3 + k;
    if (k == 0) { *ya = *y; *xa = *x; *yb = *y; *xb = *x - 1; return true; }
    if (*y % TILE_H == 0) return false;                // y == 0 included
    if (k == 1) { *ya = *y; *xa = *x; *yb = *y - 1; *xb = *x - 1; }
    else { *ya = *y; *xa = *x - 1; *yb = *y - 1; *xb = *x; }
    return true;
}
CC_HD bool border_pair(int conn, int H, int W, long slot, int* ya, int* xa, int* yb, int* xb) {
    int kind, y, x;
    return border_pair(conn, H, W, slot, ya, xa, yb, xb, &kind, &y, &x);
}

// A pair both of whose pixels are members need not be united when other pairs of the same enumeration, together with the
// neighbours already joined inside their tiles, connect its pixels anyway -- the rule of tile_unite_pixel along the edge.
// mem(y, x): membership, asked only inside the image.  A horizontal-edge pair leans only on neighbours in its own tile column and
// on horizontal-edge pairs further left there, a vertical-edge pair only on its own tile row and on vertical-edge pairs further
// up: no pair is dropped because of a pair that is dropped because of it.
//   kind 0: the pixel to the left and ITS upper neighbour are members (that pair joins the same two tile components)
//   kind 1, 2: the upper neighbour is a member (the diagonal one lies beside it), or the pixel below the diagonal one is
//   kind 3: the pixels above both are members;  kind 4, 5: one of the other two pixels of the 2 x 2 square is a member
template <class M>
CC_HD bool pair_redundant(int kind, int y, int x, int W, const M& mem) {
    const bool same_l = x % TILE_W != 0, same_r = (x + 1) % TILE_W != 0 && x + 1 < W, same_u = y % TILE_H != 0;
    switch (kind) {
        case 0: return same_l && mem(y, x - 1) && mem(y - 1, x - 1);
        case 1: return same_l && (mem(y - 1, x) || mem(y, x - 1));
        case 2: return same_r && (mem(y - 1, x) || mem(y, x + 1));
        case 3: return same_u && mem(y - 1, x) && mem(y - 1, x - 1);
        case 4: return mem(y, x - 1) || mem(y - 1, x);          // (these two kinds exist only where same_u holds)
        default: return mem(y, x) || mem(y - 1, x - 1);
    }
}

// ---- one tile (local pixel i = ly * TILE_W + lx).  A tile row is 64 pixels: with its membership as a bit mask, every pixel starts
// at the first pixel of its horizontal run -- lab[i] = tile_init(row mask, ly, lx), the forest after all left-right unions, with
// no union made -- and -1 at a non-member.
static_assert(TILE_W == 64, "a tile row is one 64-bit membership mask");
CC_HD int tile_init(unsigned long long row, int ly, int lx) {
    if (!((row >> lx) & 1ull)) return -1;
    const unsigned long long gaps = ~row & ((1ull << lx) - 1ull);       // the non-members left of lx
    return ly * TILE_W + (gaps ? 64 - __builtin_clzll(gaps) : 0);
}
// The unions of pixel i with the row above, inside the tile; the runs are joined already (tile_init).  Along a stretch where
// pixel and upper neighbour are both members, every vertical pair joins the same two runs: only the stretch's first pixel
// unites.  conn 8: a diagonal neighbour counts only where the upper neighbour itself is no member (else it lies in that
// neighbour's run) and where the pixel beside i below it is no member (else that pixel has it as its upper neighbour).
template <class A>
CC_HD void tile_unite_pixel(int* lab, int i, int conn) {
    const int ly = i / TILE_W, lx = i % TILE_W, u = i - TILE_W;
    if (ly == 0 || A::load(lab + i) < 0) return;
    const bool left = lx > 0 && A::load(lab + i - 1) >= 0, right = lx < TILE_W - 1 && A::load(lab + i + 1) >= 0;
    const bool ul = lx > 0 && A::load(lab + u - 1) >= 0, ur = lx < TILE_W - 1 && A::load(lab + u + 1) >= 0;
    if (A::load(lab + u) >= 0) {
        if (!(left && ul)) unite<A>(lab, i, u);
        return;
    }
    if (conn != 8) return;
    if (ul && !left) unite<A>(lab, i, u - 1);
    if (ur && !right) unite<A>(lab, i, u + 1);
}
// the plane's node of the tile's local pixel r (tile origin y0, x0)
CC_HD int tile_node(int r, int y0, int x0, int W) { return node((long)(y0 + r / TILE_W) * W + x0 + r % TILE_W); }

// ---- the filter: component of `size` pixels in a plane of `total` foreground pixels is removed when size / total < num / den
// (the reference: 1 / 5; products in 64 bits; num = 0 removes nothing)
CC_HD bool removed(long long size, long long total, int num, int den) { return (long long)den * size < (long long)num * total; }

}  // namespace cc
}  // namespace ustrun
